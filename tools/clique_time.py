#!/usr/bin/env python3
"""Time of the batched max-clique + TLS estimator at the 3DMatch shape: B = 1 and 64 pairs of second-level clouds of ~10 k points with
~3 000 matches each (the pairs of tools/fgr_time.py), on two inputs -- 20 % false rows (a clique of ~2 400 members: the walks are long)
and 5 % true rows (a clique of ~150: the walks are 15 x shorter) -- beside the three other estimators of the classical row on the same
matches in the same session.

    python tools/clique_time.py [--pairs 1,64] [--matches 3000] [--repeats 10] [--out FILE.json]

Reports ms per call, median and min..max over the repeats after a warm-up, HIP events around each call, for
    clique          ops.clique_batched with d_thr = tim_thr = inlier_thr = 1.5 voxels, t_thr = half of it (what FpfhRegistration passes)
    sc2             ops.sc2_batched as tools/sc2_time.py runs it
    fgr             ops.fgr_batched as tools/fgr_time.py runs it
    ransac_loop     fpfh.ransac_on_matches pair by pair at cfg.ransac_hypotheses
and, from a separate pass with the library's timing registry on (events between the stages of one call), the stages of clique:
graph (gather, bit matrix, degrees), peel, order (+ the second bit matrix), walks, pose (GNC-TLS + voting), polish.
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

STAGES = dict(graph=19, peel=20, order=21, walks=22, pose=23, polish=24)                      # BUF_TIMED_CLIQUE_* of buffer_hip.h
INPUTS = dict(false20=0.8, true5=0.05)                                                        # name -> share of true rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', default='1,64')
    ap.add_argument('--matches', type=int, default=3000)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('clique_time: no HIP device (a time is measured on the GPU or not at all)')
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

    out = dict(tool='clique_time', matches=a.matches, ransac_hypotheses=int(cfg.ransac_hypotheses), d_thr=thr, inputs={})
    for name, true_frac in INPUTS.items():
        out['inputs'][name] = {}
        for B in [int(x) for x in a.pairs.split(',')]:
            src_h, sl, tgt_h, tl, corr_h, cl, poses = make_pairs(B, a.matches, true_frac=true_frac)
            src, tgt, corr = (torch.from_numpy(x).to(dev) for x in (src_h, tgt_h, corr_h))
            so, to, co = (np.concatenate([[0], np.cumsum(x)]) for x in (sl, tl, cl))
            seeds = list(range(B))
            views = [(src[so[b]:so[b + 1]], tgt[to[b]:to[b + 1]], corr[co[b]:co[b + 1]].contiguous()) for b in range(B)]
            fns = dict(clique=lambda: ops.clique_batched(src, sl, tgt, tl, corr, cl, thr),
                       sc2=lambda: ops.sc2_batched(src, sl, tgt, tl, corr, cl, thr, thr),
                       fgr=lambda: ops.fgr_batched(src, sl, tgt, tl, corr, cl, seeds, delta=thr, delta_absolute=True),
                       ransac_loop=lambda: [fpfh.ransac_on_matches(s, t, c, cfg.ransac_hypotheses, seeds[b], thr, 0.9)
                                            for b, (s, t, c) in enumerate(views)])
            t, res = {k: [] for k in fns}, {}
            for it in range(a.warmup + a.repeats):
                for k, fn in fns.items():
                    ms, res[k] = timed(fn)
                    if it >= a.warmup:
                        t[k].append(ms)
            L.buf_timing_enable(1)                                # the stages, in a pass of their own: the events cost a little
            for kid in STAGES.values():
                collect(kid)
            for _ in range(a.repeats):
                fns['clique']()
            torch.cuda.synchronize()
            stages = {k: collect(kid) for k, kid in STAGES.items()}
            L.buf_timing_enable(0)
            info = res['clique'][1].cpu().numpy()
            X = dict(clique=res['clique'][0].cpu().numpy(), sc2=res['sc2'][0].cpu().numpy(), fgr=res['fgr'][0].cpu().numpy(),
                     ransac_loop=np.stack([p.cpu().numpy().astype(np.float64) for p in res['ransac_loop']]))

            def good(T):                                          # pairs within 15 degrees and 0.3 m of the known motion
                cosv = np.clip((np.einsum('bij,bij->b', T[:, :3, :3], poses[:, :3, :3]) - 1) / 2, -1, 1)
                return int(((np.degrees(np.arccos(cosv)) < 15) & (np.linalg.norm(T[:, :3, 3] - poses[:, :3, 3], axis=1) < 0.3)).sum())

            out['inputs'][name][str(B)] = dict(
                points=int(sl.sum()), **{k: stats(v, B) for k, v in t.items()}, stages_mean_ms=stages,
                bound_mean=float(info[:, 2].mean()), clique_mean=float(info[:, 3].mean()), gnc_steps_mean=float(info[:, 6].mean()),
                inliers_mean=float(info[:, 7].mean()), status_ok=int((info[:, 0] == 1).sum()),
                certified=int(((info[:, 0] == 1) & (info[:, 2] == info[:, 3])).sum()), registered={k: good(v) for k, v in X.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
