#!/usr/bin/env python3
"""Time of the ISS keypoint detector at the 3DMatch shape: the 64 second-level clouds of ~10 k points of tools/fpfh_time.py (planar
room surfaces on a jittered 3.5 cm lattice, shuffled), salient radius 0.21 and non-max radius 0.14 (6 and 4 voxels of 0.035).

    python tools/iss_time.py [--clouds 64] [--repeats 20] [--out FILE.json]

Reports the k chosen for each radius (the longest row: whole rows), the keypoints per cloud, and ms per call, median and min..max
over the repeats after a warm-up, for
    grid_build       ops.CellGrid over the stacked clouds at the salient radius               (HIP events around the call)
    count_queries    the two count-only queries that size k, with their read-back             (HIP events around the call)
    query_salient    the self query at the salient radius, k = its longest row                (HIP events around the call)
    query_non_max    the self query at the non-max radius                                     (HIP events around the call)
    saliency, nms    k_iss_saliency and k_iss_nms, each bracketed by HIP events inside buf_iss_keypoints (buf_timing_enable, ids 25, 26)
    iss_keypoints    keypoints.iss_keypoints end to end, compaction included                  (HIP events around the call)
    spfh_same_rows   k_spfh on the first --spfh-k columns of the salient rows (id 12), beside saliency_same_rows = k_iss_saliency on the
                     same columns (max_nn = --spfh-k): the two kernels at equal k
Needs a HIP device; prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
BUF_TIMED_SPFH, BUF_TIMED_ISS_SALIENCY, BUF_TIMED_ISS_NMS = 12, 25, 26


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clouds', type=int, default=64)
    ap.add_argument('--salient-radius', type=float, default=0.21)
    ap.add_argument('--non-max-radius', type=float, default=0.14)
    ap.add_argument('--spfh-k', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('iss_time: no HIP device (a time is measured on the GPU or not at all)')
    from buffer_amd import _lib, keypoints, ops
    from fpfh_time import make_clouds, stats
    dev = torch.device('cuda:0')
    L = _lib.lib()
    pts_h, nrm_h, lens = make_clouds(a.clouds)
    pts, nrm = torch.from_numpy(pts_h).to(dev), torch.from_numpy(nrm_h).to(dev)
    n = int(pts.shape[0])
    rs, rn = a.salient_radius, a.non_max_radius

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

    names = ('grid_build', 'count_queries', 'query_salient', 'query_non_max', 'saliency', 'nms', 'iss_keypoints', 'spfh_same_rows',
             'saliency_same_rows')
    t = {k: [] for k in names}
    for it in range(a.warmup + a.repeats):
        tb, grid = timed(lambda: ops.CellGrid(pts, lens, max(rs, rn)))
        tc, (ks, kn) = timed(lambda: keypoints._whole_row_k(grid, pts, lens, [rs, rn]))
        tqs, nbr_sal = timed(lambda: grid.query(pts, lens, ks, radius=rs, q_order=grid.order))
        tqn, nbr_nms = timed(lambda: grid.query(pts, lens, kn, radius=rn, q_order=grid.order))
        L.buf_timing_enable(1)
        mask, sal, eig = ops.iss_keypoints(pts, nbr_sal, nbr_nms)
        tsal, tnms = collect(BUF_TIMED_ISS_SALIENCY), collect(BUF_TIMED_ISS_NMS)
        ops.fpfh(pts, nrm, nbr_sal, a.spfh_k)
        tspfh = collect(BUF_TIMED_SPFH)
        L.buf_timing_collect_kernel(13, None, None)
        ops.iss_keypoints(pts, nbr_sal, nbr_nms, max_nn=a.spfh_k)
        tsame = collect(BUF_TIMED_ISS_SALIENCY)
        L.buf_timing_collect_kernel(BUF_TIMED_ISS_NMS, None, None)
        L.buf_timing_enable(0)
        te, (idx, counts) = timed(lambda: keypoints.iss_keypoints(pts, rs, rn, lengths=lens))
        if it >= a.warmup:
            for k, v in zip(names, (tb, tc, tqs, tqn, tsal, tnms, te, tspfh, tsame)):
                t[k].append(v)
    assert torch.equal(idx, torch.nonzero(mask).reshape(-1)) and torch.isfinite(sal).all() and torch.isfinite(eig).all()
    cs, cn = (nbr_sal < n).sum(1).cpu().numpy(), (nbr_nms < n).sum(1).cpu().numpy()
    out = dict(tool='iss_time', clouds=a.clouds, points=n, salient_radius=rs, non_max_radius=rn, k_salient=ks, k_non_max=kn,
               row_mean_salient=float(cs.mean()), row_mean_non_max=float(cn.mean()), rows_mb=(ks + kn) * 4.0 * n / 1e6, spfh_k=a.spfh_k,
               keypoints_total=int(counts.sum()), keypoints_per_cloud_mean=float(counts.mean()),
               keypoints_per_cloud_min=int(counts.min()), keypoints_per_cloud_max=int(counts.max()),
               **{k: stats(v) for k, v in t.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
