"""ICP on KITTI-shape ring scans before voxelisation (synth.make_kitti_pair(raw=True), ~120k returns per scan), the way
kitti.KittiTestSet refines its ground truth (0.20 m, <= 200 iterations, relative criteria 1e-6): icp.icp_batched at batch 1
(one pair per call, as icp.icp_point_to_point runs it) and at batch --pairs.  The source scan starts from the true pose
perturbed by a small error (odometry is close, not exact).  Times are HIP-event spans after a warm-up of every path.
--method point_to_plane / generalized: the same runs with that step; the 30-NN normals they need (targets / all scans, ONE stacked
preprocess.estimate_normals call) are timed as a span of their own, normals_ms, outside the ICP spans.
--method voxelized [--voxel V] [--neighbors K]: voxelized Generalized ICP (icp.vgicp_batched); the map build and the loop on a
prebuilt map are spans of their own.  --repeats R: every span (the normals excepted) is the median of R runs.
Prints one JSON line:  python tools/icp_time.py [--pairs 16] [--method point_to_point]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buffer_amd import icp, ops, preprocess, synth  # noqa: E402


REPEATS = [1]


def _span(fn):
    """-> (fn's result, the median HIP-event span in ms of --repeats runs)"""
    ms = []
    for _ in range(REPEATS[0]):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--max-iteration', type=int, default=200)
    ap.add_argument('--dist', type=float, default=0.20)
    ap.add_argument('--method', default='point_to_point', choices=sorted(ops.ICP_METHODS) + ['voxelized'])
    ap.add_argument('--epsilon', type=float, default=1e-3, help='generalized / voxelized: the covariance along a normal')
    ap.add_argument('--voxel', type=float, default=None, help='voxelized: the voxel edge (default: twice --dist)')
    ap.add_argument('--neighbors', type=int, default=7, choices=ops.VGICP_NEIGHBORS, help='voxelized: voxels met by a source point')
    ap.add_argument('--repeats', type=int, default=1, help='timed runs per span after the warm-up; the median is reported')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    srcs, tgts = [], []
    for seed in range(a.pairs):
        s = synth.make_kitti_pair(seed, raw=True)
        e = np.deg2rad(rng.uniform(-0.3, 0.3, 3))
        cz, sz, cy, sy = np.cos(e[2]), np.sin(e[2]), np.cos(e[1]), np.sin(e[1])
        E = np.eye(4)
        E[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        E[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        M = E @ s['relt_pose']                                               # "odometry": the true pose with a small error
        xyz0 = s['src_raw'] @ M[:3, :3].T + M[:3, 3]
        srcs.append(torch.from_numpy(xyz0.astype(np.float32)).to(dev))
        tgts.append(torch.from_numpy(s['tgt_raw'].astype(np.float32)).to(dev))
    def normals(clouds):
        """one stacked estimate_normals call -> one array per cloud"""
        n = [c.shape[0] for c in clouds]
        return list(torch.split(preprocess.estimate_normals(torch.cat(clouds), knn=30, orient=False, lengths=n), n))

    need = dict(point_to_point=[], point_to_plane=tgts, generalized=srcs + tgts, voxelized=srcs + tgts)[a.method]
    nrm, t_normals = [], 0.0
    if need:
        normals(need)                                                        # warm-up
        nrm, t_normals = _span(lambda: normals(need))
    REPEATS[0] = max(a.repeats, 1)
    if a.method == 'voxelized':
        return voxelized(a, srcs, tgts, nrm, t_normals)

    def extra(lo, hi):
        """the method's arguments for pairs lo..hi-1"""
        if a.method == 'point_to_plane':
            return dict(tgt_normals=nrm[lo:hi])
        if a.method == 'generalized':
            return dict(src_normals=nrm[lo:hi], tgt_normals=nrm[len(srcs) + lo:len(srcs) + hi], epsilon=a.epsilon)
        return {}

    kw = dict(method=a.method, max_iteration=a.max_iteration)
    # warm-up of both paths (code objects, allocator)
    icp.icp_batched(srcs[:1], tgts[:1], a.dist, **dict(kw, max_iteration=3), **extra(0, 1))
    icp.icp_batched(srcs, tgts, a.dist, **dict(kw, max_iteration=3), **extra(0, len(srcs)))

    one, t_one = [], 0.0
    for b, (s, t) in enumerate(zip(srcs, tgts)):
        r, ms = _span(lambda: icp.icp_batched([s], [t], a.dist, **kw, **extra(b, b + 1))[0])
        one.append(r); t_one += ms
    batch, t_batch = _span(lambda: icp.icp_batched(srcs, tgts, a.dist, **kw, **extra(0, len(srcs))))
    it1, itb = [r['iterations'] for r in one], [r['iterations'] for r in batch]
    B = len(srcs)
    print(json.dumps(dict(
        method=a.method, normals_ms=t_normals, pairs=B, points_per_scan=int(np.mean([s.shape[0] for s in srcs])), max_dist=a.dist, max_iteration=a.max_iteration,
        batch1_ms_per_pair=t_one / B, batch1_ms_per_iteration=t_one / max(sum(it1), 1),
        batched_ms_per_pair=t_batch / B, batched_ms_per_pair_iteration=t_batch / max(sum(itb), 1),
        batched_rounds=max(itb) + 1, iterations_batched=itb,
        iterations_batch1_equal_batched=it1 == itb,
        max_abs_T_diff_batch1_vs_batched=float(max(np.abs(x['T'] - y['T']).max() for x, y in zip(one, batch))))))


def voxelized(a, srcs, tgts, nrm, t_normals):
    """--method voxelized: the map build (one map of all targets; one map per target for the batch-1 runs) and the loop on a PREBUILT
    map are spans of their own: the loop span is what a second call on the same targets costs, the map span what reuse saves."""
    B = len(srcs)
    voxel = 2.0 * a.dist if a.voxel is None else a.voxel
    sn, tn = nrm[:B], nrm[B:]
    kw = dict(neighbors=a.neighbors, max_iteration=a.max_iteration)
    icp.vgicp_batched(srcs[:1], icp.voxel_map(tgts[:1], voxel, tn[:1], a.epsilon), src_normals=sn[:1], **dict(kw, max_iteration=3))   # warm-up
    icp.vgicp_batched(srcs, icp.voxel_map(tgts, voxel, tn, a.epsilon), src_normals=sn, **dict(kw, max_iteration=3))
    maps, t_map1 = [], 0.0
    for b in range(B):
        m, ms = _span(lambda: icp.voxel_map(tgts[b:b + 1], voxel, tn[b:b + 1], a.epsilon))
        maps.append(m); t_map1 += ms
    vmap, t_map = _span(lambda: icp.voxel_map(tgts, voxel, tn, a.epsilon))
    one, t_one = [], 0.0
    for b in range(B):
        r, ms = _span(lambda: icp.vgicp_batched(srcs[b:b + 1], maps[b], src_normals=sn[b:b + 1], **kw)[0])
        one.append(r); t_one += ms
    batch, t_batch = _span(lambda: icp.vgicp_batched(srcs, vmap, src_normals=sn, **kw))
    it1, itb = [r['iterations'] for r in one], [r['iterations'] for r in batch]
    print(json.dumps(dict(
        method=a.method, voxel=voxel, neighbors=a.neighbors, normals_ms=t_normals, pairs=B, points_per_scan=int(np.mean([s.shape[0] for s in srcs])),
        max_iteration=a.max_iteration, map_rows=vmap.nrows, batch1_map_ms_per_pair=t_map1 / B, batched_map_ms_per_pair=t_map / B,
        batch1_ms_per_pair=t_one / B, batch1_ms_per_iteration=t_one / max(sum(it1), 1),
        batched_ms_per_pair=t_batch / B, batched_ms_per_pair_iteration=t_batch / max(sum(itb), 1),
        batched_rounds=max(itb) + 1, iterations_batched=itb, iterations_batch1_equal_batched=it1 == itb,
        mean_fitness=float(np.mean([r['fitness'] for r in batch])),
        max_abs_T_diff_batch1_vs_batched=float(max(np.abs(x['T'] - y['T']).max() for x, y in zip(one, batch))))))


if __name__ == '__main__':
    main()
