#!/usr/bin/env python3
"""Time of the k-NN search on the cell grid (ops.grid_knn, csrc/knn3.hip, include/buffer_hip.h N14) and of what sits on it
(preprocess.knn_search, the two outlier filters, estimate_normals_knn), in one session, at the two shapes of tools/normals_time.py:

    kitti      2 x --pairs raw KITTI-shape ring scans of ~120 k returns
    3dmatch    --clouds second-level clouds of ~10 k points on a jittered 3.5 cm lattice

    python tools/knn_time.py [--pairs 16] [--clouds 64] [--repeats 10] [--warmup 2] [--shapes kitti 3dmatch] [--out FILE.json]

Per shape and k = 2, 20, 30, ms per call (median, min..max over the repeats after the warm-ups, HIP events around the call):
    grid_knn        the kernel alone on a grid built at the pilot's radius (the median k-th distance), in the grid's order; edge_median =
                    the cell edge the build took (coarsened where a cloud's box does not fit its share of the table)
    knn_search      pilot + grid build + kernel
and, from that k's rows, ring1 = the share of queries whose k-th neighbour lies closer than the nearest face of the 27-cell cube around
their cell (a lower bound of the share the kernel closes after ring 1: faces of the grid itself would not count), ring0 the same for the
query's own cell.  Then
    statistical     remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0)
    radius          remove_radius_outlier(nb_points=16, radius = the pilot's 20th-neighbour distance)
    normals_knn, normals_knn30, normals_radius      estimate_normals_knn(30), estimate_normals(knn=30) and estimate_normals_radius(radius of
                    normals_time.py, max_nn=30) on the same points, and the largest / 99th-percentile / median angle between the first two.
Needs a HIP device; prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), repeats=int(ms.size))


def measure(a, pts, lens, normal_radius, dev):
    import torch
    from buffer_amd import _lib, ops, preprocess

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
    out = dict(points=n, clouds=len(lens))
    seg = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.as_tensor(lens, dtype=torch.int64, device=dev))
    clouds = torch.split(pts, [int(m) for m in lens])
    mn_c = torch.stack([c.min(0).values for c in clouds]).double()
    ext_c = (torch.stack([c.max(0).values for c in clouds]).double() - mn_c).cpu().numpy()
    mn = mn_c[seg]
    cells = _lib.lib().buf_grid_default_cells(n, len(lens))      # the table share CellGrid gives every cloud
    for k in (2, 20, 30):
        cell = preprocess._knn_pilot_cell(pts, lens, k)
        grid = ops.CellGrid(pts, lens, cell)
        row = dict(pilot_cell=cell)
        row['grid_knn'], (nbr, d2) = span(lambda: grid.knn(pts, lens, k, q_order=grid.order, return_d2=True))
        row['knn_search'], (nbr2, _) = span(lambda: preprocess.knn_search(pts, k, lens))
        assert torch.equal(nbr, nbr2)
        # the edge the build really took per cloud: the pilot's, coarsened by 1.25 until the cloud's box fits its table share
        edges = np.array([ops.grid_cell_dims(e, cell, cells)[0] for e in ext_c])
        row.update(edge_median=float(np.median(edges)), coarsened_clouds=int((edges > cell * 1.0001).sum()))
        edge = torch.from_numpy(edges).to(dev)[seg]
        f = (pts.double() - mn) / edge[:, None]
        fr = f - torch.floor(f)
        m = torch.minimum(fr, 1.0 - fr).min(1).values
        kth = d2[:, k - 1].double().sqrt()
        row['ring0'] = float((kth < m * edge).double().mean())
        row['ring1'] = float((kth < (1.0 + m) * edge).double().mean())
        row['median_query_inside_ring1'] = bool(row['ring1'] >= 0.5)
        out[f'k{k}'] = row
    out['statistical'], (keep, _, _, _) = span(lambda: preprocess.remove_statistical_outlier(pts, 20, 2.0, lengths=lens))
    out['statistical_removed'] = float(1.0 - keep.double().mean())
    r = preprocess._knn_pilot_cell(pts, lens, 20)
    out['radius'], (keep, _) = span(lambda: preprocess.remove_radius_outlier(pts, 16, r, lengths=lens))
    out.update(radius_removed=float(1.0 - keep.double().mean()), radius_filter_radius=r)
    out['normals_knn'], nk = span(lambda: preprocess.estimate_normals_knn(pts, 30, orient=False, lengths=lens))
    out['normals_knn30'], n30 = span(lambda: preprocess.estimate_normals(pts, knn=30, orient=False, lengths=lens))
    out['normals_radius'], _ = span(lambda: preprocess.estimate_normals_radius(pts, normal_radius, 30, orient=False, lengths=lens))
    ang = torch.rad2deg(torch.acos((nk.double() * n30.double()).sum(1).abs().clamp(max=1.0)))
    out['angle_knn_vs_knn30_deg'] = dict(max=float(ang.max()), p99=float(torch.quantile(ang[:10_000_000], 0.99)), median=float(ang.median()),
                                         above_1_deg=int((ang > 1.0).sum()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', type=int, default=16, help='kitti: pairs of scans (2 scans each)')
    ap.add_argument('--clouds', type=int, default=64, help='3dmatch: clouds')
    ap.add_argument('--kitti-dist', type=float, default=0.20, help='kitti: the radius of normals_radius is twice it (normals_time.py)')
    ap.add_argument('--voxel', type=float, default=0.035, help='3dmatch: the voxel; the radius of normals_radius is twice it')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--shapes', nargs='+', default=['kitti', '3dmatch'], choices=['kitti', '3dmatch'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('knn_time: no HIP device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = dict(tool='knn_time', warmup=a.warmup, repeats=a.repeats)
    if '3dmatch' in a.shapes:
        import fpfh_time
        pts_h, _, lens = fpfh_time.make_clouds(a.clouds, voxel=a.voxel)
        out['3dmatch'] = measure(a, torch.from_numpy(pts_h).to(dev), np.asarray(lens, np.int32), 2.0 * a.voxel, dev)
    if 'kitti' in a.shapes:
        import normals_time
        srcs, tgts = normals_time.kitti_scans(a.pairs, dev)
        clouds = srcs + tgts
        lens = np.array([c.shape[0] for c in clouds], np.int32)
        out['kitti'] = measure(a, torch.cat(clouds).contiguous(), lens, 2.0 * a.kitti_dist, dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
