#!/usr/bin/env python3
"""Time of batched SC2-PCR at the 3DMatch shape: B = 1 and 64 pairs of second-level clouds of ~10 k points with ~3 000 matches each, a
third of them true (the pairs of tools/fgr_time.py), beside the two other estimators of the classical row on the same matches in the
same session.

    python tools/sc2_time.py [--pairs 1,64] [--matches 3000] [--repeats 20] [--out FILE.json]

Reports ms per call, median and min..max over the repeats after a warm-up, HIP events around each call, for
    sc2             ops.sc2_batched with d_thr = inlier_thr = 1.5 voxels and the defaults (what FpfhRegistration passes)
    fgr             ops.fgr_batched as tools/fgr_time.py runs it
    ransac_loop     fpfh.ransac_on_matches pair by pair at cfg.ransac_hypotheses
and, from a separate pass with the library's timing registry on (events between the stages of one call), the stages of sc2:
compatibility (gather + bit matrix), confidence (power iteration, suppression, seeds), counts, hypotheses, refinement.
Needs a HIP device; prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

STAGES = dict(compatibility=14, confidence=15, counts=16, hypotheses=17, refinement=18)      # BUF_TIMED_SC2_* of buffer_hip.h


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', default='1,64')
    ap.add_argument('--matches', type=int, default=3000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sc2_time: no HIP device (a time is measured on the GPU or not at all)')
    from buffer_amd import _lib, fpfh, ops
    from buffer_amd.config import THREEDMATCH as cfg
    from fgr_time import make_pairs, stats
    L = _lib.lib()
    dev = torch.device('cuda:0')
    thr = 1.5 * cfg.voxel_size_0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def collect(kid):
        ms, work = C.c_double(0), C.c_double(0)
        n = L.buf_timing_collect_kernel(kid, C.byref(ms), C.byref(work))
        return ms.value / max(n, 1)

    out = dict(tool='sc2_time', matches=a.matches, ransac_hypotheses=int(cfg.ransac_hypotheses), d_thr=thr, batches={})
    for B in [int(x) for x in a.pairs.split(',')]:
        src_h, sl, tgt_h, tl, corr_h, cl, poses = make_pairs(B, a.matches)
        src, tgt, corr = (torch.from_numpy(x).to(dev) for x in (src_h, tgt_h, corr_h))
        so, to, co = (np.concatenate([[0], np.cumsum(x)]) for x in (sl, tl, cl))
        seeds = list(range(B))
        views = [(src[so[b]:so[b + 1]], tgt[to[b]:to[b + 1]], corr[co[b]:co[b + 1]].contiguous()) for b in range(B)]
        sc2 = lambda: ops.sc2_batched(src, sl, tgt, tl, corr, cl, thr, thr)
        fgr = lambda: ops.fgr_batched(src, sl, tgt, tl, corr, cl, seeds, delta=thr, delta_absolute=True)
        loop = lambda: [fpfh.ransac_on_matches(s, t, c, cfg.ransac_hypotheses, seeds[b], thr, 0.9) for b, (s, t, c) in enumerate(views)]
        t = dict(sc2=[], fgr=[], ransac_loop=[])
        for it in range(a.warmup + a.repeats):
            ts, res = timed(sc2)
            tf, fres = timed(fgr)
            tr, rposes = timed(loop)
            if it >= a.warmup:
                t['sc2'].append(ts)
                t['fgr'].append(tf)
                t['ransac_loop'].append(tr)
        L.buf_timing_enable(1)                                    # the stages, in a pass of their own: the events cost a little
        for kid in STAGES.values():
            collect(kid)
        for _ in range(a.repeats):
            sc2()
        torch.cuda.synchronize()
        stages = {k: collect(kid) for k, kid in STAGES.items()}
        L.buf_timing_enable(0)
        T, info = res[0].cpu().numpy(), res[1].cpu().numpy()
        F = fres[0].cpu().numpy()
        R = np.stack([p.cpu().numpy().astype(np.float64) for p in rposes])

        def good(X):                                              # pairs within 15 degrees and 0.3 m of the known motion
            cosv = np.clip((np.einsum('bij,bij->b', X[:, :3, :3], poses[:, :3, :3]) - 1) / 2, -1, 1)
            return int(((np.degrees(np.arccos(cosv)) < 15) & (np.linalg.norm(X[:, :3, 3] - poses[:, :3, 3], axis=1) < 0.3)).sum())

        out['batches'][str(B)] = dict(points=int(sl.sum()), **{k: stats(v, B) for k, v in t.items()}, stages_mean_ms=stages,
                                      seeds_mean=float(info[:, 2].mean()), inliers_mean=float(info[:, 5].mean()),
                                      status_ok=int((info[:, 0] == 1).sum()), sc2_registered=good(T), fgr_registered=good(F),
                                      ransac_registered=good(R))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
