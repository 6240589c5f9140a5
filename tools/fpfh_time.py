#!/usr/bin/env python3
"""Time of the FPFH descriptor at the 3DMatch shape: 64 second-level clouds of ~10 k points (planar room surfaces sampled on a
jittered 3.5 cm lattice, shuffled), radius 0.175, max_nn 100.

    python tools/fpfh_time.py [--clouds 64] [--repeats 20] [--out FILE.json]

Reports ms per call, median and min..max over the repeats after a warm-up, for
    grid_build      ops.CellGrid over the stacked clouds                                  (HIP events around the call)
    grid_query      the self query with k = max_nn in the grid's order                     (HIP events around the call)
    spfh, fpfh      k_spfh and k_fpfh, each bracketed by HIP events inside buf_fpfh        (buf_timing_enable, ids 12 and 13)
    compute_fpfh    fpfh.compute_fpfh end to end                                           (HIP events around the call)
and the effective bandwidth of k_fpfh's SPFH gather: 264 bytes (one f64[33] row) per WEIGHTED neighbour, counted from the rows
themselves, over the kernel's median time, beside the HBM peak.  Needs a HIP device; prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TBS = 8.0                 # MI355X HBM3E, specification
HBM_COPY_TBS = 6.3                 # what a streaming copy reaches on it
BUF_TIMED_SPFH, BUF_TIMED_FPFH = 12, 13


def make_clouds(nclouds, seed=0, voxel=0.035):
    """-> (points f32[n,3], normals f32[n,3], lengths): per cloud a floor and two walls on a jittered lattice, shuffled"""
    rng = np.random.default_rng(seed)
    pts, nrm, lens = [], [], []
    for _ in range(nclouds):
        a, b, h = rng.uniform(2.3, 2.9), rng.uniform(2.3, 2.9), rng.uniform(0.9, 1.3)
        parts = []
        for (lu, lv, o, eu, ev, nr) in ((a, b, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)), (a, h, (0, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0)),
                                        (b, h, (0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0))):
            u, v = np.meshgrid(np.arange(0, lu, voxel), np.arange(0, lv, voxel), indexing='ij')
            uv = np.stack([u.ravel(), v.ravel()], 1) + rng.uniform(-0.3, 0.3, (u.size, 2)) * voxel
            p = np.asarray(o, np.float64) + uv[:, :1] * np.asarray(eu, np.float64) + uv[:, 1:] * np.asarray(ev, np.float64)
            p += rng.normal(scale=0.002, size=p.shape)
            parts.append((p, np.tile(np.asarray(nr, np.float64), (len(p), 1))))
        p, q = np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])
        perm = rng.permutation(len(p))
        pts.append(p[perm] + rng.uniform(-5, 5, 3))
        nrm.append(q[perm])
        lens.append(len(p))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32), np.array(lens, np.int32)


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), repeats=int(ms.size))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clouds', type=int, default=64)
    ap.add_argument('--radius', type=float, default=0.175)
    ap.add_argument('--max-nn', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fpfh_time: no HIP device (a time is measured on the GPU or not at all)')
    from buffer_amd import _lib, fpfh, ops
    dev = torch.device('cuda:0')
    L = _lib.lib()
    pts_h, nrm_h, lens = make_clouds(a.clouds)
    pts, nrm = torch.from_numpy(pts_h).to(dev), torch.from_numpy(nrm_h).to(dev)
    n = int(pts.shape[0])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def collect(kid):
        ms, work = C.c_double(0), C.c_double(0)
        k = L.buf_timing_collect_kernel(kid, C.byref(ms), C.byref(work))
        assert k == 1, k
        return ms.value

    t = dict(grid_build=[], grid_query=[], spfh=[], fpfh=[], compute_fpfh=[])
    nbr = None
    for it in range(a.warmup + a.repeats):
        tb, grid = timed(lambda: ops.CellGrid(pts, lens, a.radius))
        tq, nbr = timed(lambda: grid.query(pts, lens, a.max_nn, q_order=grid.order))
        L.buf_timing_enable(1)
        ops.fpfh(pts, nrm, nbr, a.max_nn)
        ts, tf = collect(BUF_TIMED_SPFH), collect(BUF_TIMED_FPFH)
        L.buf_timing_enable(0)
        tc, F = timed(lambda: fpfh.compute_fpfh(pts, nrm, a.radius, a.max_nn, lens))
        if it >= a.warmup:
            for k, v in zip(('grid_build', 'grid_query', 'spfh', 'fpfh', 'compute_fpfh'), (tb, tq, ts, tf, tc)):
                t[k].append(v)
    # the gather, counted from the rows: every column 1.. that holds a point (no two points of these clouds coincide, so each has a weight)
    assert len(np.unique(pts_h, axis=0)) == n
    cnt = (nbr < n).sum(1).cpu().numpy()
    weighted = int((nbr[:, 1:] < n).sum().item())
    gather_bytes = 264.0 * weighted
    out = dict(tool='fpfh_time', clouds=a.clouds, points=n, radius=a.radius, max_nn=a.max_nn, row_mean=float(cnt.mean()), row_max=int(cnt.max()),
               rows_full=float((cnt >= a.max_nn).mean()), weighted_neighbours=weighted, spfh_table_mb=n * 264 / 1e6,
               **{k: stats(v) for k, v in t.items()})
    tbs = gather_bytes / (out['fpfh']['median_ms'] * 1e-3) / 1e12
    out['fpfh_gather'] = dict(bytes=gather_bytes, tb_per_s=tbs, of_hbm_peak=tbs / HBM_PEAK_TBS, of_hbm_copy=tbs / HBM_COPY_TBS,
                              arithmetic=f'264 B x {weighted} weighted neighbours / {out["fpfh"]["median_ms"]:.4f} ms; HBM peak {HBM_PEAK_TBS} TB/s '
                                         f'(specification), {HBM_COPY_TBS} TB/s (streaming copy)')
    assert torch.isfinite(F).all()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
