"""ETH test-set driver: the data side of generalization/ThreeD2ETH and KITTI2ETH on top of the device pipeline
(counterpart of ThreeD2ETH/dataset.py:25-119, dataloader.py and test.py:47-87; KITTI2ETH/test.py reads the same set).

    <root>/<scene>/Hokuyo_<i>.ply      fragments (terrestrial laser scans, each in its own scanner frame)
    <root>/<scene>/gt.log              pairs and poses, in the 3DMatch .log format (plyio.load_gt_log)

The set is registered with the constants of a cross-dataset preset (3DMatch or KITTI weights; buffer_amd/config.py) and
scored by the DGR criterion of ThreeD2ETH/test.py:65-72: RTE < 0.3 m and RRE < 2 degrees.  Host code is file IO and
bookkeeping only; voxelisation, normals and registration run on the device (buffer_amd.preprocess, buffer_amd.pipeline)."""
import os

import numpy as np

from . import driver, evaluate
from .plyio import load_gt_log, read_ply

SCENES = ['gazebo_summer', 'gazebo_winter', 'wood_autmn', 'wood_summer']      # dataset.py:34-39 (the reference's spelling)
DGR_THRESHOLDS = (0.3, 2.0)                                                   # RTE m, RRE degrees (ThreeD2ETH/test.py:65-72)


class ETHTestSet(driver.PairTestSet):
    """ETHTestset (dataset.py:25-52): the (src, tgt, gt) of every scene's gt.log, scene by scene in file order."""

    def __init__(self, root, scenes=None, downsample=0.05, voxel_size_0=0.15, max_num_pts=30000):
        self.root = root
        self.downsample, self.voxel_size_0, self.max_num_pts = downsample, voxel_size_0, max_num_pts
        self.scenes = list(SCENES if scenes is None else scenes)
        self.files, self.poses = [], []
        for scene in self.scenes:
            sdir = os.path.join(root, scene)
            if not os.path.isdir(sdir):
                raise FileNotFoundError(f'ETH scene directory {sdir} not found')
            if not os.path.isfile(os.path.join(sdir, 'gt.log')):
                raise FileNotFoundError(f'ETH ground truth {os.path.join(sdir, "gt.log")} not found')
            for key, pose in load_gt_log(sdir).items():             # key 'i_j': source Hokuyo_i, target Hokuyo_j
                i, j = key.split('_')
                self.files.append((os.path.join(scene, f'Hokuyo_{i}'), os.path.join(scene, f'Hokuyo_{j}')))
                self.poses.append(pose)

    def scene(self, index):
        return self.files[index][0].split(os.sep)[0]

    def raw_pair(self, index):
        """the two scans of pair `index` as read from disk, non-finite rows dropped (open3d's read_point_cloud defaults):
        (f32[n,3], f32[m,3]) numpy"""
        return tuple(read_ply(os.path.join(self.root, fid + '.ply'), drop_non_finite=True) for fid in self.files[index])

    def meta(self, index, device=None):
        src_id, tgt_id = self.files[index]
        return {'src_id': src_id, 'tgt_id': tgt_id, 'relt_pose': np.linalg.inv(self.poses[index])}      # dataset.py:76


def register_pairs(pipe, dataset, indices, batch=32, stage_metrics=False):
    """driver.register_pairs at this driver's default batch"""
    return driver.register_pairs(pipe, dataset, indices, batch, stage_metrics)


def summarize(dataset, poses, rte_thresh=DGR_THRESHOLDS[0], rre_thresh=DGR_THRESHOLDS[1]):
    """DGR recall / TE / RE of ThreeD2ETH/test.py:65-87 (and KITTI2ETH/test.py:64-72): success = RTE < 0.3 m and RRE < 2 deg;
    TE / RE are means over the successful pairs (NaN when none).  poses f32[n,4,4] in dataset order.
    -> dict(pairs, recall, te, re, per_scene={scene: recall})."""
    stats = [evaluate.dgr_success(poses[i], dataset.meta(i)['relt_pose'], rte_thresh, rre_thresh) for i in range(len(dataset))]
    good = np.array([s[0] for s in stats], bool)
    scene_of = np.array([dataset.scene(i) for i in range(len(dataset))], dtype=object)
    per_scene = {s: float(good[scene_of == s].mean()) if (scene_of == s).any() else 0.0 for s in dataset.scenes}
    return dict(driver.dgr_summary(stats), per_scene=per_scene)


def parse_args(argv=None):
    """the command line of main() -> (args, Config of --preset)"""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    driver.add_common_args(ap, 'eth', 8, 'log_ETH')
    ap.add_argument('--scenes', nargs='+', default=None, help='default: ' + ' '.join(SCENES))
    return driver.parse_with_preset(ap, argv, 'eth')


def main(argv=None):
    """python -m buffer_amd.eth --root <ETH root> [--preset 3DMatch->ETH|KITTI->ETH]   (one process per GPU under torchrun).
    Prints one JSON line (rank 0) and returns the poses f32[n,4,4] (numpy) on rank 0."""
    a, cfg = parse_args(argv)
    ranks = driver.init()
    ds = ETHTestSet(a.root, a.scenes, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
    return driver.run(a, cfg, ds, ranks, calibrate_pairs=8, dgr_thresholds=DGR_THRESHOLDS, log_root=a.log_root or 'log_ETH',
                      summarize=lambda poses: summarize(ds, poses), scene_of=[ds.scene(i) for i in range(len(ds))],
                      labels=[f'{s} {t}' for s, t in ds.files])


if __name__ == '__main__':
    main()
