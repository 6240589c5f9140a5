"""ETH test-set driver: the data side of generalization/ThreeD2ETH and KITTI2ETH on top of the device pipeline
(counterpart of ThreeD2ETH/dataset.py:25-119, dataloader.py and test.py:47-87; KITTI2ETH/test.py reads the same set).

    <root>/<scene>/Hokuyo_<i>.ply      fragments (terrestrial laser scans, each in its own scanner frame)
    <root>/<scene>/gt.log              pairs and poses, in the 3DMatch .log format (threedmatch.load_gt_log)

The set is registered with the constants of a cross-dataset preset (3DMatch or KITTI weights; buffer_amd/config.py) and
scored by the DGR criterion of ThreeD2ETH/test.py:65-72: RTE < 0.3 m and RRE < 2 degrees.  Host code is file IO and
bookkeeping only; voxelisation, normals and registration run on the device (buffer_amd.preprocess, buffer_amd.pipeline)."""
import os

import numpy as np
import torch

from . import evaluate, preprocess
from .threedmatch import load_gt_log, read_ply, register_pairs, stage_report   # register_pairs: the batched path of the 3DMatch driver

SCENES = ['gazebo_summer', 'gazebo_winter', 'wood_autmn', 'wood_summer']      # dataset.py:34-39 (the reference's spelling)


class ETHTestSet:
    """ETHTestset (dataset.py:25-52): the (src, tgt, gt) of every scene's gt.log, scene by scene in file order.
    Duck type of threedmatch.ThreeDMatchTestSet, so threedmatch.items_batched / register_pairs and
    BufferPipeline.register_batches take it unchanged."""

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

    def __len__(self):
        return len(self.files)

    def scene(self, index):
        return self.files[index][0].split(os.sep)[0]

    def raw_pair(self, index):
        """the two scans of pair `index` as read from disk, non-finite rows dropped (open3d's read_point_cloud defaults):
        (f32[n,3], f32[m,3]) numpy"""
        return tuple(read_ply(os.path.join(self.root, fid + '.ply'), drop_non_finite=True) for fid in self.files[index])

    def meta(self, index, device=None):
        src_id, tgt_id = self.files[index]
        return {'src_id': src_id, 'tgt_id': tgt_id, 'relt_pose': np.linalg.inv(self.poses[index])}      # dataset.py:76

    def item(self, index, device, seed=None):
        """dataset.py:54-115: read both scans, two voxel levels, shuffles, cap, 30-NN normals -- on the device.
        -> the sample dict of the reference, holding DEVICE tensors (+ src_id, tgt_id, relt_pose)."""
        out = self.meta(index)
        for j, raw in enumerate(self.raw_pair(index)):
            side = ('src', 'tgt')[j]
            it = preprocess.prepare_fragment(torch.from_numpy(raw).to(device), self.downsample, self.voxel_size_0, self.max_num_pts,
                                             seed=2 * index + j if seed is None else seed)
            out[f'{side}_fds_pts'], out[f'{side}_sds_pts'] = it['fds_pts'], it['sds_pts']
        return out


def summarize(dataset, poses, rte_thresh=0.3, rre_thresh=2.0):
    """DGR recall / TE / RE of ThreeD2ETH/test.py:65-87 (and KITTI2ETH/test.py:64-72): success = RTE < 0.3 m and RRE < 2 deg;
    TE / RE are means over the successful pairs (NaN when none).  poses f32[n,4,4] in dataset order.
    -> dict(pairs, recall, te, re, per_scene={scene: recall})."""
    st = np.array([evaluate.dgr_success(poses[i], dataset.meta(i)['relt_pose'], rte_thresh, rre_thresh) for i in range(len(dataset))],
                  np.float64).reshape(-1, 3)
    good = st[:, 0] == 1
    scene_of = np.array([dataset.scene(i) for i in range(len(dataset))], dtype=object)
    per_scene = {s: float(good[scene_of == s].mean()) if (scene_of == s).any() else 0.0 for s in dataset.scenes}
    return dict(pairs=int(st.shape[0]), recall=float(good.mean()) if st.size else 0.0,
                te=float(st[good, 1].mean()) if good.any() else float('nan'),
                re=float(st[good, 2].mean()) if good.any() else float('nan'), per_scene=per_scene)


def parse_args(argv=None):
    """the command line of main() -> (args, Config of --preset)"""
    import argparse

    from .config import DRIVER_PRESETS, preset
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument('--root', required=True)
    ap.add_argument('--preset', default=DRIVER_PRESETS['eth'][0],
                    help='constants and weights (buffer_amd/config.py): ' + ', '.join(DRIVER_PRESETS['eth']))
    ap.add_argument('--scenes', nargs='+', default=None, help='default: ' + ' '.join(SCENES))
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--limits', default=None, help='frozen neighbourhood limits "a,b,c" (default: calibrate like dataloader.py:18-51)')
    ap.add_argument('--stage-metrics', action='store_true',
                    help='also compute the per-stage ground-truth metrics (repeatability, inlier ratio, FMR, consensus precision): '
                         'summary key "stage", per-pair rows in <log-root>/stage_metrics.json')
    ap.add_argument('--log-root', default=None, help='where --stage-metrics writes stage_metrics.json (default: log_ETH)')
    ap.add_argument('--by-overlap', action='store_true',
                    help='also compute every pair\'s overlap under the ground truth (buffer_amd/pairs.py) and report pair count, DGR recall '
                         'and, with --stage-metrics, the stage figures per overlap band: summary key "by_overlap"')
    a = ap.parse_args(argv)
    try:
        cfg = preset(a.preset, 'eth')
    except ValueError as e:
        ap.error(str(e))
    return a, cfg


def main(argv=None):
    """python -m buffer_amd.eth --root <ETH root> [--preset 3DMatch->ETH|KITTI->ETH]   (one process per GPU under torchrun).
    Prints one JSON line (rank 0) and returns the poses f32[n,4,4] (numpy) on rank 0."""
    import json
    import time

    import torch.distributed as dist

    from . import dist as bdist
    from .pipeline import BufferPipeline
    a, cfg = parse_args(argv)
    rank, world, dev, cdev = bdist.init(int(os.environ.get('LOCAL_RANK', 0)))
    ds = ETHTestSet(a.root, a.scenes, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
    pipe = BufferPipeline(cfg, dev)
    if a.limits:
        pipe.limits = [int(x) for x in a.limits.split(',')]
    else:
        if rank == 0:                                        # dataloader.py:18-51 on the first pairs
            host = []
            for i in range(min(len(ds), 8)):
                s = ds.item(i, dev)
                host.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in s.items()})
            pipe.calibrate(host)
        pipe.limits = bdist.broadcast_limits(pipe.limits if rank == 0 else [0, 0, 0], device=cdev)
    ids = bdist.shard_indices(len(ds), rank, world)
    t0 = time.perf_counter()
    res = register_pairs(pipe, ds, ids, a.batch, stage_metrics=a.stage_metrics)
    poses = bdist.gather_poses(ids, res[0] if a.stage_metrics else res, len(ds), device=cdev)
    counts = bdist.gather_counts(ids, res[1].to(cdev), len(ds), device=cdev).cpu().numpy() if a.stage_metrics else None
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    poses = poses.cpu().numpy()
    if rank == 0:
        out = summarize(ds, poses)
        out.update(preset=a.preset, pairs_per_sec=len(ds) / dt, n_gpus=world, limits=pipe.limits)
        overlaps = None
        if a.by_overlap:
            from . import pairs
            out['by_overlap'], overlaps = pairs.overlap_report(ds, poses, dev, 0.3, 2.0, counts, cfg.num_keypts)       # (summarize's thresholds)
        if a.stage_metrics:
            out['stage'] = stage_report([ds.scene(i) for i in range(len(ds))], counts, cfg.num_keypts)
            evaluate.write_stage_metrics(os.path.join(a.log_root or 'log_ETH', 'stage_metrics.json'), [f'{s} {t}' for s, t in ds.files],
                                         counts, cfg.num_keypts, out['stage'], overlaps)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()
    return poses if rank == 0 else None


if __name__ == '__main__':
    main()
