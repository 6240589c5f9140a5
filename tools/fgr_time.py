#!/usr/bin/env python3
"""Time of batched Fast Global Registration at the 3DMatch shape: B = 1, 16 and 64 pairs of second-level clouds of ~10 k points (the
room surfaces of tools/fpfh_time.py; the target is the moved copy with 2 mm noise), each pair with ~3 000 matches of which a third
are true and the rest go to random target rows -- the mix a mutual FPFH match list has.

    python tools/fgr_time.py [--pairs 1,16,64] [--matches 3000] [--repeats 20] [--out FILE.json]

Reports ms per call, median and min..max over the repeats after a warm-up, HIP events around each call, for
    fgr             ops.fgr_batched with open3d's defaults, the paper's delta = 1.5 voxels (what FpfhRegistration passes)
    fgr_tuples      the same call with iterations = 0: the tuple test and the normalisation alone (k_fgr_tuples + the head of
                    k_fgr_optimize); fgr - fgr_tuples is the share of the 64 Gauss-Newton steps
    ransac_loop     the present estimator on the same matches: fpfh.ransac_on_matches pair by pair at cfg.ransac_hypotheses
and per pair.  Needs a HIP device; prints one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def make_pairs(npairs, matches, seed=0, true_frac=1 / 3, noise=0.002):
    """-> (src f32[.,3], src lengths, tgt f32[.,3], tgt lengths, corr int32[.,2], corr lengths, poses f64[B,4,4])"""
    from fpfh_time import make_clouds
    rng = np.random.default_rng(seed + 1)
    pts, _, lens = make_clouds(npairs, seed)
    off = np.concatenate([[0], np.cumsum(lens)])
    tgt, corr, poses = [], [], []
    for b in range(npairs):
        p = pts[off[b]:off[b + 1]].astype(np.float64)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        ang = rng.uniform(0.3, 1.2)
        T = np.eye(4)
        T[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
        T[:3, 3] = rng.uniform(-1, 1, 3)
        tgt.append((p @ T[:3, :3].T + T[:3, 3] + rng.normal(scale=noise, size=p.shape)).astype(np.float32))
        rows = rng.choice(len(p), size=matches, replace=False)
        to = rows.copy()
        false = rng.random(matches) >= true_frac
        to[false] = rng.integers(0, len(p), int(false.sum()))
        corr.append(np.stack([np.sort(rows), to[np.argsort(rows)]], 1).astype(np.int32))
        poses.append(T)
    return pts, lens, np.concatenate(tgt), lens.copy(), np.concatenate(corr), np.full(npairs, matches, np.int32), np.stack(poses)


def stats(ms, B):
    ms = np.asarray(ms, np.float64)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), repeats=int(ms.size),
                median_ms_per_pair=float(np.median(ms)) / B)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', default='1,16,64')
    ap.add_argument('--matches', type=int, default=3000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fgr_time: no HIP device (a time is measured on the GPU or not at all)')
    from buffer_amd import fpfh, ops
    from buffer_amd.config import THREEDMATCH as cfg
    dev = torch.device('cuda:0')
    delta = 1.5 * cfg.voxel_size_0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    out = dict(tool='fgr_time', matches=a.matches, ransac_hypotheses=int(cfg.ransac_hypotheses), delta=delta, batches={})
    for B in [int(x) for x in a.pairs.split(',')]:
        src_h, sl, tgt_h, tl, corr_h, cl, poses = make_pairs(B, a.matches)
        src, tgt, corr = (torch.from_numpy(x).to(dev) for x in (src_h, tgt_h, corr_h))
        so, to, co = (np.concatenate([[0], np.cumsum(x)]) for x in (sl, tl, cl))
        seeds = list(range(B))
        views = [(src[so[b]:so[b + 1]], tgt[to[b]:to[b + 1]], corr[co[b]:co[b + 1]].contiguous()) for b in range(B)]
        run = lambda it: ops.fgr_batched(src, sl, tgt, tl, corr, cl, seeds, delta=delta, delta_absolute=True, iterations=it)
        loop = lambda: [fpfh.ransac_on_matches(s, t, c, cfg.ransac_hypotheses, seeds[b], delta, 0.9) for b, (s, t, c) in enumerate(views)]
        t = dict(fgr=[], fgr_tuples=[], ransac_loop=[])
        res = None
        for it in range(a.warmup + a.repeats):
            tf, res = timed(lambda: run(64))
            tt, _ = timed(lambda: run(0))
            tr, rposes = timed(loop)
            if it >= a.warmup:
                t['fgr'].append(tf)
                t['fgr_tuples'].append(tt)
                t['ransac_loop'].append(tr)
        T, info = res[0].cpu().numpy(), res[1].cpu().numpy()
        R = np.stack([p.cpu().numpy().astype(np.float64) for p in rposes])

        def good(X):                                              # pairs within 15 degrees and 0.3 m of the known motion
            cosv = np.clip((np.einsum('bij,bij->b', X[:, :3, :3], poses[:, :3, :3]) - 1) / 2, -1, 1)
            return int(((np.degrees(np.arccos(cosv)) < 15) & (np.linalg.norm(X[:, :3, 3] - poses[:, :3, 3], axis=1) < 0.3)).sum())

        out['batches'][str(B)] = dict(points=int(sl.sum()), **{k: stats(v, B) for k, v in t.items()},
                                      optimisation_share=1.0 - float(np.median(t['fgr_tuples'])) / float(np.median(t['fgr'])),
                                      trials_mean=float(info[:, 2].mean()), tuples_mean=float(info[:, 1].mean()),
                                      status_ok=int((info[:, 0] == 1).sum()), fgr_registered=good(T), ransac_registered=good(R))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
