"""3DMatch / 3DLoMatch test-set driver: the data side of ThreeDMatch/test.py on top of the device pipeline
(counterpart of ThreeDMatch/dataset.py:47-76,80-162 test split, utils/tools.py:6-7,47-62, test.py:199-308).

    <root>/test/3DMatch/fragments/<scene>/cloud_bin_<k>.ply        fragments
    <root>/test/3DMatch/gt_result/<scene>/gt.log, gt.info          pairs, ground-truth poses, information matrices
    <root>/test/3DLoMatch/<scene>/gt.log, gt.info                  (3DLoMatch pairs over the same fragments)

Host code is file IO and bookkeeping only; voxelisation, normals and registration run on the device
(buffer_amd.preprocess, buffer_amd.pipeline)."""
import os

import numpy as np

from . import driver, evaluate
from .driver import items_batched, stage_report, upload      # noqa: F401  (kept importable from here)
from .plyio import load_gt_log, read_ply, write_ply          # noqa: F401  (kept importable from here)

SCENES = ['7-scenes-redkitchen', 'sun3d-home_at-home_at_scan1_2013_jan_1', 'sun3d-home_md-home_md_scan9_2012_sep_30',
          'sun3d-hotel_uc-scan3', 'sun3d-hotel_umd-maryland_hotel1', 'sun3d-hotel_umd-maryland_hotel3',
          'sun3d-mit_76_studyroom-76-1studyroom2', 'sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika']   # dataset.py:49-58
DGR_THRESHOLDS = (0.3, 15.0)                                 # RTE m, RRE degrees (test.py:263-270)


class ThreeDMatchTestSet(driver.PairTestSet):
    """ThreeDMatchDataset(split='test') (dataset.py:47-76): the list of (src, tgt, gt) of every scene's gt.log."""

    def __init__(self, root, dataset='3DMatch', scenes=None, downsample=0.02, voxel_size_0=0.035, max_num_pts=30000):
        self.root = os.path.join(root, 'test')
        self.dataset = dataset
        self.gt_root = os.path.join(self.root, dataset, 'gt_result') if dataset == '3DMatch' else os.path.join(self.root, dataset)
        self.downsample, self.voxel_size_0, self.max_num_pts = downsample, voxel_size_0, max_num_pts
        self.files, self.poses = [], []
        for scene in (SCENES if scenes is None else scenes):
            gt = load_gt_log(os.path.join(self.gt_root, scene))
            frag = os.path.join('3DMatch', 'fragments', scene)
            for key, pose in gt.items():
                i, j = key.split('_')
                self.files.append((os.path.join(frag, f'cloud_bin_{i}'), os.path.join(frag, f'cloud_bin_{j}')))
                self.poses.append(pose)

    def raw_pair(self, index):
        """the two fragments of pair `index` as read from disk: (f32[n,3], f32[m,3]) numpy"""
        return tuple(read_ply(os.path.join(self.root, fid + '.ply')) for fid in self.files[index])

    def meta(self, index, device=None):
        src_id, tgt_id = self.files[index]
        return {'src_id': src_id, 'tgt_id': tgt_id, 'relt_pose': np.linalg.inv(self.poses[index])}      # dataset.py:122


def register_pairs(pipe, dataset, indices, batch=32, stage_metrics=False):
    """driver.register_pairs at this driver's default batch"""
    return driver.register_pairs(pipe, dataset, indices, batch, stage_metrics)


def write_logs(dataset, poses, log_root, log_name):
    """test.py:242-270 over all pairs in dataset order: append the inverse pose to <log_root>/<scene>/<log_name>
    and collect the DGR statistics.  poses f32[n,4,4].  -> list of (success, rte, rre)."""
    stats = []
    for i, (src_id, tgt_id) in enumerate(dataset.files):
        T = np.asarray(poses[i], dtype=np.float64)
        scene = src_id.split(os.sep)[-2]
        evaluate.append_log(os.path.join(log_root, scene, log_name), src_id.split('_')[-1], tgt_id.split('_')[-1], T)
        stats.append(evaluate.dgr_success(T, np.linalg.inv(dataset.poses[i]), *DGR_THRESHOLDS))
    return stats


def summarize(dataset, stats, log_root, log_name):
    """DGR recall / TE / RE (test.py:278-284) and the Registration Recall over the scenes' logs (:287-308)."""
    rr, per_scene = evaluate.registration_recall(dataset.gt_root, log_root, log_name)
    return dict(driver.dgr_summary(stats, 'dgr_recall'), registration_recall=rr, per_scene=[float(x) for x in per_scene])


def parse_args(argv=None):
    """the command line of main() -> (args, Config of --preset).  --dataset defaults to the preset's target data set."""
    import argparse
    import time
    ap = argparse.ArgumentParser(description=main.__doc__)
    driver.add_common_args(ap, 'threedmatch', 32, 'log_<dataset>', ' (generalization/KITTI2ThreeD: KITTI weights on the 3DLoMatch pairs)')
    ap.add_argument('--dataset', default=None, choices=['3DMatch', '3DLoMatch'], help="default: the preset's target data set")
    ap.add_argument('--log-name', default=time.strftime('%m%d%H%M') + '.log')
    a, cfg = driver.parse_with_preset(ap, argv, 'threedmatch')
    if a.dataset is None:
        a.dataset = cfg.dataset
    return a, cfg


def main(argv=None):
    """python -m buffer_amd.threedmatch --root <data root> [--preset KITTI->3DLoMatch] [--dataset 3DLoMatch]   (one process per GPU
    under torchrun).  Returns the poses f32[n,4,4] (numpy) on rank 0."""
    a, cfg = parse_args(argv)
    ranks = driver.init()
    ds = ThreeDMatchTestSet(a.root, a.dataset, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
    log_root = a.log_root or f'log_{a.dataset}'
    return driver.run(a, cfg, ds, ranks, calibrate_pairs=8, dgr_thresholds=DGR_THRESHOLDS, log_root=log_root,
                      summarize=lambda poses: summarize(ds, write_logs(ds, poses, log_root, a.log_name), log_root, a.log_name),
                      scene_of=[f[0].split(os.sep)[-2] for f in ds.files], labels=[f'{s} {t}' for s, t in ds.files])


if __name__ == '__main__':
    main()
