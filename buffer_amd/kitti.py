"""KITTI odometry test driver: the data side of KITTI/test.py on top of the device pipeline
(counterpart of KITTI/dataset.py:23-118,196-226 test split and KITTI/test.py:43-88).

    <root>/dataset/sequences/<dd>/velodyne/<tttttt>.bin     scans (float32 x, y, z, reflectance)
    <root>/dataset/poses/<dd>.txt                            camera-0 odometry, 12 numbers per frame
    <root>/icp/<drive>_<t0>_<t1>.npy                         ICP-refined ground truth (optional cache)

`python -m buffer_amd.kitti --root R --refine-gt` fills that cache in batches on the device (KittiTestSet.refine_ground_truths)
and exits; run it first so that a timed run starts from a full cache.

The reference refines the odometry ground truth with open3d ICP on first use and caches it under icp/
(dataset.py:95-117); here the cached file is used when present, otherwise the same ICP refinement runs on the device
(buffer_amd/icp.py::icp_batched) and fills the cache; --allow-odometry-gt skips the refinement.  The summary reports how many pairs used
which source (`gt_source`).  Host code is file IO and bookkeeping; voxelisation, normals and registration run on the device."""
import glob
import json
import os
import time

import numpy as np
import torch

from . import dist as bdist, driver, evaluate

TEST_DRIVES = (8, 9, 10)                                            # KITTI/test_kitti.txt
DGR_THRESHOLDS = (0.3, 1.0)                                         # RTE m, RRE degrees (KITTI/test.py:66-88)
VELO2CAM = np.vstack((np.hstack([np.array([7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01,
                                           9.998621e-01, 7.523790e-03, 1.480755e-02]).reshape(3, 3),
                                 np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01]).reshape(3, 1)]), [0, 0, 0, 1])).T   # dataset.py:203-213


def odometry_to_positions(odometry):
    """dataset.py:216-219"""
    return np.vstack((odometry.reshape(3, 4), [0, 0, 0, 1]))


def select_pairs(scan_ids, positions, min_dist=10.0, window=100):
    """Test pairs of one drive (the rule of KITTI/dataset.py:52-67): starting from the first scan t, the partner is
    the LAST frame before the vehicle has moved more than `min_dist` metres from t (searched over the next `window`
    frames of the pose table); the following pair starts right after the partner.  A frame with no such partner in
    the window is skipped.  positions f64[n_frames,3] (camera-0 translations), scan_ids = frames that have a scan.
    Distances are taken against frame t only (O(window) per step, not the full n x n table)."""
    have = set(int(i) for i in scan_ids)
    pairs, t = [], int(min(have))
    while t in have:
        d = np.sqrt(((positions[t:t + window] - positions[t]) ** 2).sum(-1))
        far = np.flatnonzero(d > min_dist)
        partner = t + int(far[0]) - 1 if far.size else None
        if partner is not None and partner in have:
            pairs.append((t, partner))
            t = partner + 1
        else:
            t += 1          # no partner in the window (or its scan file is missing): move on
    return pairs


class KittiTestSet(driver.PairTestSet):
    """KITTIDataset(split='test') (dataset.py:44-70): scan pairs about 10 m apart along the trajectory."""

    def __init__(self, root, drives=TEST_DRIVES, downsample=0.05, voxel_size_0=0.30, max_num_pts=40000,
                 allow_odometry_gt=False):
        self.pc_path = os.path.join(root, 'dataset')
        self.icp_path = os.path.join(root, 'icp')
        self.downsample, self.voxel_size_0, self.max_num_pts = downsample, voxel_size_0, max_num_pts
        self.allow_odometry_gt = allow_odometry_gt
        self.gt_source = {}                                          # pair index -> 'icp-cache' | 'odometry'
        self.files, self._odo = [], {}
        for drive in drives:
            fnames = glob.glob(os.path.join(self.pc_path, 'sequences', '%02d' % drive, 'velodyne', '*.bin'))
            if not fnames:
                raise FileNotFoundError(f'no velodyne scans for drive {drive} under {self.pc_path}')
            scan_ids = [int(os.path.basename(f)[:-4]) for f in fnames]
            positions = np.array([odometry_to_positions(o)[:3, 3] for o in self.odometry(drive)])
            self.files += [(drive, t0, t1) for t0, t1 in select_pairs(scan_ids, positions)]
        if (8, 15, 58) in self.files:                                # "pair (8, 15, 58) is wrong" (dataset.py:69-71)
            self.files.remove((8, 15, 58))

    def odometry(self, drive):
        if drive not in self._odo:
            self._odo[drive] = np.genfromtxt(os.path.join(self.pc_path, 'poses', '%02d.txt' % drive)).reshape(-1, 12)
        return self._odo[drive]

    def scan(self, drive, t):
        fn = os.path.join(self.pc_path, 'sequences', '%02d' % drive, 'velodyne', '%06d.bin' % t)
        return np.ascontiguousarray(np.fromfile(fn, dtype=np.float32).reshape(-1, 4)[:, :3])

    def _odometry_transform(self, index):
        """the odometry transform M of scan t0 -> scan t1 (dataset.py:100-102)"""
        drive, t0, t1 = self.files[index]
        p0, p1 = (odometry_to_positions(o) for o in self.odometry(drive)[[t0, t1]])
        return (VELO2CAM @ p0.T @ np.linalg.inv(p1.T) @ np.linalg.inv(VELO2CAM)).T

    def ground_truth(self, index, device=None):
        """dataset.py:95-117: transform scan t0 -> scan t1.  The reference refines the odometry transform M with
        point-to-point ICP on the raw scans (threshold 0.20 m, <= 200 iterations), stores `M @ T_icp` under
        icp/<drive>_<t0>_<t1>.npy and evaluates against that.  Here: the cached file if present; otherwise the same
        refinement on the device (refine_ground_truths, needs `device`), written to the same cache; the raw odometry
        transform only with `allow_odometry_gt`.  Every pair's source is recorded in `gt_source`."""
        cached = os.path.join(self.icp_path, '%d_%d_%d.npy' % self.files[index])
        if not os.path.exists(cached):
            if self.allow_odometry_gt:
                self.gt_source[index] = 'odometry'
                return self._odometry_transform(index)
            if device is None:
                raise FileNotFoundError(f'{cached} missing: the reference evaluates against ICP-refined poses; call with a device '
                                        f'to refine here, or pass allow_odometry_gt=True (--allow-odometry-gt) for raw odometry')
            self.refine_ground_truths([index], device)
        if self.gt_source.get(index) != 'icp-device':                 # (a file this object refined itself keeps its label)
            self.gt_source[index] = 'icp-cache'
        return np.load(cached)

    def refine_ground_truths(self, indices, device, batch=16):
        """Fill the icp/ cache for every listed pair whose file is missing, `batch` pairs per buf_icp_batched call
        (buffer_amd/icp.py::icp_batched): odometry transform M, point-to-point ICP of the raw scans at 0.20 m,
        <= 200 iterations, `M @ T_icp` (the reference's composition order, dataset.py:110).  A pair's result does not depend
        on the batch, so a file has the same bits whichever call wrote it.  Existing cache files are left alone; refined pairs
        are labelled 'icp-device'.  Returns the indices refined."""
        from . import icp
        todo = [i for i in indices if not os.path.exists(os.path.join(self.icp_path, '%d_%d_%d.npy' % self.files[i]))]
        for lo in range(0, len(todo), max(int(batch), 1)):
            chunk = todo[lo:lo + max(int(batch), 1)]
            Ms, srcs, tgts = [], [], []
            for i in chunk:
                drive, t0, t1 = self.files[i]
                M = self._odometry_transform(i)
                xyz0 = self.scan(drive, t0).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
                Ms.append(M)
                srcs.append(torch.from_numpy(xyz0.astype(np.float32)).to(device))
                tgts.append(torch.from_numpy(self.scan(drive, t1)).to(device))
            res = icp.icp_batched(srcs, tgts, 0.20, max_iteration=200)
            os.makedirs(self.icp_path, exist_ok=True)
            for i, M, r in zip(chunk, Ms, res):
                np.save(os.path.join(self.icp_path, '%d_%d_%d.npy' % self.files[i]), M @ r['T'])
                self.gt_source[i] = 'icp-device'
        return todo

    def raw_pair(self, index):
        drive, t0, t1 = self.files[index]
        return self.scan(drive, t0), self.scan(drive, t1)

    def meta(self, index, device=None):
        drive, t0, t1 = self.files[index]
        return {'src_id': f'{drive:02d}/{t0:06d}', 'tgt_id': f'{drive:02d}/{t1:06d}', 'relt_pose': self.ground_truth(index, device)}


def register_pairs(pipe, dataset, indices, batch=4, stage_metrics=False):
    """driver.register_pairs at this driver's default batch"""
    return driver.register_pairs(pipe, dataset, indices, batch, stage_metrics)


def summarize(dataset, poses, rte_thresh=DGR_THRESHOLDS[0], rre_thresh=DGR_THRESHOLDS[1]):
    """KITTI/test.py:66-88 (note: 0.3 m / 1 degree in the reference's script)."""
    out = driver.dgr_summary([evaluate.dgr_success(poses[i], dataset.ground_truth(i), rte_thresh, rre_thresh) for i in range(len(dataset))])
    src = list(dataset.gt_source.values())
    out['gt_source'] = {k: src.count(k) for k in ('icp-cache', 'icp-device', 'odometry')}
    return out


def parse_args(argv=None):
    """the command line of main() -> (args, Config of --preset)"""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    driver.add_common_args(ap, 'kitti', 4, 'log_KITTI', ' (generalization/ThreeD2KITTI: 3DMatch weights, scale 10)')
    ap.add_argument('--allow-odometry-gt', action='store_true',
                    help='evaluate against raw odometry instead of refining it by ICP where <root>/icp/<drive>_<t0>_<t1>.npy is missing')
    ap.add_argument('--refine-gt', action='store_true',
                    help='only fill the ICP ground-truth cache <root>/icp/ (this rank\'s shard, --batch-icp pairs per call) and exit')
    ap.add_argument('--batch-icp', type=int, default=16)
    return driver.parse_with_preset(ap, argv, 'kitti')


def main(argv=None):
    """python -m buffer_amd.kitti --root <data root> [--preset 3DMatch->KITTI]   (one process per GPU under torchrun).
    Returns the poses f32[n,4,4] (numpy) on rank 0."""
    a, cfg = parse_args(argv)
    ranks = rank, world, dev, _ = driver.init()
    ds = KittiTestSet(a.root, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts,
                      allow_odometry_gt=a.allow_odometry_gt)
    if a.refine_gt:
        ids = bdist.shard_indices(len(ds), rank, world)
        t0 = time.perf_counter()
        done = ds.refine_ground_truths(ids, dev, a.batch_icp)
        print(json.dumps(dict(rank=rank, pairs=len(ids), refined=len(done), seconds=time.perf_counter() - t0)))
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    return driver.run(a, cfg, ds, ranks, calibrate_pairs=4, dgr_thresholds=DGR_THRESHOLDS, log_root=a.log_root or 'log_KITTI',
                      summarize=lambda poses: summarize(ds, poses), labels=['%d %d %d' % f for f in ds.files])


if __name__ == '__main__':
    main()
