#!/usr/bin/env python3
"""Time of the radius / hybrid normals (preprocess.estimate_normals_radius, csrc/normals.hip, include/buffer_hip.h N13) beside the 30-NN
path (preprocess.estimate_normals), in one session, at two shapes:

    kitti      the raw KITTI-shape ring scans of tools/icp_time.py: 2 x --pairs scans of ~120 k returns (synth.make_kitti_pair(raw=True));
               radius = twice icp_time's correspondence distance (what refine_batch(normals='hybrid') takes by default)
    3dmatch    the second-level clouds of tools/fpfh_time.py: --clouds clouds of ~10 k points on a jittered 3.5 cm lattice; radius = 2 voxels

    python tools/normals_time.py [--pairs 16] [--clouds 64] [--repeats 20] [--warmup 3] [--shapes kitti 3dmatch] [--no-refine] [--out FILE.json]

Per shape, ms per call (median, min..max over the repeats after the warm-ups, HIP events around the call):
    knn30             estimate_normals(knn=30): the yardstick, the retry loop over grids
    hybrid            estimate_normals_radius(radius, max_nn=30): grid build + one query + one launch
    hybrid_given_grid the same on a caller's grid (the one FPFH or ISS built anyway)
    radius            the pure radius form, max_nn=None (one count-only query and its host wait more); skipped, with the row length it
                      would need, where the whole rows would take more than --max-row-gb of memory
    grid_build, grid_query, kernel      the three parts of `hybrid`
    kernel_<rows>_<order>               the kernel alone with direct row loads / the LDS tile (BUF_N13_ROWS), in the grid's cell order /
                                        in input order (order = null)
and the median and 99th-percentile angle between the 30-NN and the hybrid normals of the same points (printed, not judged).
kitti also: BufferPipeline.refine_batch(method='voxelized' | 'generalized') at --pairs pairs with normals='knn' and normals='hybrid', whole
calls (host waits included: wall clock around the call and a device synchronisation), unless --no-refine.
Needs a HIP device; prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), repeats=int(ms.size))


def kitti_scans(pairs, dev):
    """icp_time's scans: the source moved by the true pose with a small error -> (list of source tensors, list of target tensors)"""
    import torch
    from buffer_amd import synth
    rng = np.random.default_rng(0)
    srcs, tgts = [], []
    for seed in range(pairs):
        s = synth.make_kitti_pair(seed, raw=True)
        e = np.deg2rad(rng.uniform(-0.3, 0.3, 3))
        cz, sz, cy, sy = np.cos(e[2]), np.sin(e[2]), np.cos(e[1]), np.sin(e[1])
        E = np.eye(4)
        E[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        E[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        M = E @ s['relt_pose']
        srcs.append(torch.from_numpy((s['src_raw'] @ M[:3, :3].T + M[:3, 3]).astype(np.float32)).to(dev))
        tgts.append(torch.from_numpy(s['tgt_raw'].astype(np.float32)).to(dev))
    return srcs, tgts


def measure(a, pts, lens, radius, dev):
    import torch
    from buffer_amd import ops, preprocess

    def span(fn):
        ms, out = [], None
        for it in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return stats(ms), out

    n = int(pts.shape[0])
    out = dict(points=n, clouds=len(lens), search_radius=radius, max_nn=30)
    out['knn30'], knn = span(lambda: preprocess.estimate_normals(pts, knn=30, orient=False, lengths=lens))
    out['hybrid'], hyb = span(lambda: preprocess.estimate_normals_radius(pts, radius, 30, orient=False, lengths=lens))
    big = ops.CellGrid(pts, lens, 2.5 * radius)                  # a caller's grid at a larger radius (FPFH's 5 voxels beside 2)
    out['hybrid_given_grid'], given = span(lambda: preprocess.estimate_normals_radius(pts, radius, 30, orient=False, lengths=lens, grid=big))
    assert torch.equal(given, hyb)
    out['grid_build'], grid = span(lambda: ops.CellGrid(pts, lens, radius))
    out['grid_query'], nbr = span(lambda: grid.query(pts, lens, 30, radius=radius, q_order=grid.order))
    cnt = (nbr < n).sum(1)
    out.update(row_mean=float(cnt.float().mean()), rows_full=float((cnt >= 30).float().mean()), rows_below_3=int((cnt < 3).sum()))
    for rows in ('direct', 'lds'):
        os.environ['BUF_N13_ROWS'] = rows
        for name, order in (('cell_order', grid.order), ('input_order', None)):
            out[f'kernel_{rows}_{name}'], k = span(lambda: ops.row_normals(pts, nbr, order=order))
            assert torch.equal(k, hyb)
    os.environ.pop('BUF_N13_ROWS')
    out['kernel'], _ = span(lambda: ops.row_normals(pts, nbr, order=grid.order))
    mc = torch.zeros(1, dtype=torch.int32, device=dev)
    grid.query(pts, lens, 0, radius=radius, max_count=mc)
    longest = int(mc.item())
    out['longest_row'] = longest
    if 4.0 * n * longest <= a.max_row_gb * 2 ** 30:
        out['radius'], _ = span(lambda: preprocess.estimate_normals_radius(pts, radius, None, orient=False, lengths=lens))
    else:
        out['radius'] = f'skipped: whole rows of {longest} columns for {n} points exceed {a.max_row_gb} GiB'
    ang = torch.rad2deg(torch.acos((knn.double() * hyb.double()).sum(1).abs().clamp(max=1.0)))
    out['angle_knn_vs_hybrid_deg'] = dict(median=float(ang.median()), p99=float(torch.quantile(ang, 0.99)))
    return out


def refine_times(a, srcs, tgts, dist, dev):
    import torch
    from buffer_amd.config import KITTI
    from buffer_amd.pipeline import BufferPipeline
    pipe = BufferPipeline.__new__(BufferPipeline)                # refine_batch reads the device and the configuration only
    pipe.device, pipe.cfg = dev, KITTI
    inps = [dict(src_raw=s, tgt_raw=t) for s, t in zip(srcs, tgts)]
    T0 = torch.eye(4, dtype=torch.float64, device=dev).repeat(len(inps), 1, 1)
    out = {}
    for method in ('voxelized', 'generalized'):
        for normals in ('knn', 'hybrid'):
            ms = []
            for it in range(a.warmup + a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = pipe.refine_batch(inps, T0, method=method, max_dist=dist, max_iteration=30, normals=normals)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[f'{method}_{normals}'] = dict(stats(ms), mean_iterations=float(r['iterations'].float().mean()),
                                              mean_fitness=float(r['fitness'].mean()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', type=int, default=16, help='kitti: pairs of scans (2 scans each)')
    ap.add_argument('--clouds', type=int, default=64, help='3dmatch: clouds')
    ap.add_argument('--kitti-dist', type=float, default=0.20, help='kitti: the correspondence distance; the normals\' radius is twice it')
    ap.add_argument('--voxel', type=float, default=0.035, help='3dmatch: the voxel; the normals\' radius is twice it')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--shapes', nargs='+', default=['kitti', '3dmatch'], choices=['kitti', '3dmatch'])
    ap.add_argument('--no-refine', action='store_true', help='kitti: leave out the whole refine_batch calls')
    ap.add_argument('--max-row-gb', type=float, default=4.0, help='the pure radius form is skipped where its rows would take more')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('normals_time: no HIP device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = dict(tool='normals_time', warmup=a.warmup, repeats=a.repeats)
    if 'kitti' in a.shapes:
        srcs, tgts = kitti_scans(a.pairs, dev)
        clouds = srcs + tgts
        lens = np.array([c.shape[0] for c in clouds], np.int32)
        out['kitti'] = measure(a, torch.cat(clouds).contiguous(), lens, 2.0 * a.kitti_dist, dev)
        if not a.no_refine:
            out['kitti']['refine_batch'] = dict(pairs=a.pairs, max_dist=a.kitti_dist, max_iteration=30,
                                                **refine_times(a, srcs, tgts, a.kitti_dist, dev))
        del srcs, tgts, clouds
    if '3dmatch' in a.shapes:
        import fpfh_time
        pts_h, _, lens = fpfh_time.make_clouds(a.clouds, voxel=a.voxel)
        out['3dmatch'] = measure(a, torch.from_numpy(pts_h).to(dev), lens, 2.0 * a.voxel, dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
