#!/usr/bin/env python3
"""Time of the descriptor matching of the classical baseline at the shape of tools/fpfh_time.py: the FPFH descriptors (d = 33) of 64
second-level clouds of ~10 k points, i.e. 32 pairs, and of 1 pair.

    python tools/match_time.py [--clouds 64] [--repeats 10] [--out FILE.json]

Reports ms per call (wall clock between two device synchronisations: the old path synchronises the host inside, so events alone
would not see all of it), median and min..max over the repeats after a warm-up, for
    loop            fpfh.match pair by pair: two ops.knn calls and a mask per pair -- the path FpfhRegistration took before, THE YARDSTICK
    batch           ONE fpfh.match_batch call (ops.feature_match, csrc/match.hip) on the same descriptors
at 32 pairs and at 1 pair, their ratio, and the same two ways of matching inside a whole `--descriptor fpfh --estimator fgr` chunk
(FpfhRegistration.register_batch on the 32 pairs: FPFH, matching, one Fast Global Registration call), with matching's share of the
chunk before and after.  The rows of the two ways are compared before anything is timed.  Needs a HIP device; prints one JSON line."""
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clouds', type=int, default=64)
    ap.add_argument('--radius', type=float, default=0.175)
    ap.add_argument('--max-nn', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('match_time: no HIP device (a time is measured on the GPU or not at all)')
    from buffer_amd import fpfh
    from buffer_amd.config import THREEDMATCH
    from fpfh_time import make_clouds
    dev = torch.device('cuda:0')
    pts_h, nrm_h, lens = make_clouds(a.clouds - a.clouds % 2)
    pts, nrm = torch.from_numpy(pts_h).to(dev), torch.from_numpy(nrm_h).to(dev)
    F = fpfh.compute_fpfh(pts, nrm, a.radius, a.max_nn, lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    B = len(lens) // 2

    def loop(nb):
        return [fpfh.match(F[off[2 * b]:off[2 * b + 1]], F[off[2 * b + 1]:off[2 * b + 2]], True) for b in range(nb)]

    def batch(nb):
        return fpfh.match_batch(F[:off[2 * nb]], lens[:2 * nb], True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    corrs = loop(B)
    corr, cl = batch(B)
    assert cl.tolist() == [int(c.shape[0]) for c in corrs] and torch.equal(corr, torch.cat(corrs)), 'the two ways of matching differ'

    # the chunk: the dicts driver.upload makes of the pairs, through register_batch with either way of matching
    inps = [dict(points=pts[off[2 * b]:off[2 * b + 2]], features=nrm[off[2 * b]:off[2 * b + 2]], lengths=lens[2 * b:2 * b + 2]) for b in range(B)]

    class PairByPair(fpfh.FpfhRegistration):                      # FpfhRegistration as it matched before: fpfh.match per pair
        def _batch_matches(self, pts, lens, off, F):
            n = len(lens) // 2
            cs = [fpfh.match(F[int(off[2 * b]):int(off[2 * b + 1])], F[int(off[2 * b + 1]):int(off[2 * b + 2])], True) for b in range(n)]
            src = torch.cat([pts[int(off[2 * b]):int(off[2 * b + 1])] for b in range(n)])
            tgt = torch.cat([pts[int(off[2 * b + 1]):int(off[2 * b + 2])] for b in range(n)])
            return src, tgt, torch.cat(cs), [int(c.shape[0]) for c in cs]

    regs = dict(before=PairByPair(THREEDMATCH, dev, estimator='fgr'), after=fpfh.FpfhRegistration(THREEDMATCH, dev, estimator='fgr'))
    seeds = list(range(B))
    pb, pa = regs['before'].register_batch(inps, seeds), regs['after'].register_batch(inps, seeds)
    assert all(torch.equal(x, y) for x, y in zip(pb, pa)), 'the poses of the two ways of matching differ'

    t = {k: [] for k in ('loop', 'batch', 'loop_1', 'batch_1', 'chunk_before', 'chunk_after')}
    for it in range(a.warmup + a.repeats):
        row = dict(loop=timed(lambda: loop(B))[0], batch=timed(lambda: batch(B))[0], loop_1=timed(lambda: loop(1))[0],
                   batch_1=timed(lambda: batch(1))[0], chunk_before=timed(lambda: regs['before'].register_batch(inps, seeds))[0],
                   chunk_after=timed(lambda: regs['after'].register_batch(inps, seeds))[0])
        if it >= a.warmup:
            for k, v in row.items():
                t[k].append(v)
    out = dict(tool='match_time', clouds=len(lens), pairs=B, points=int(pts.shape[0]), d=int(F.shape[1]), matches=int(cl.sum()),
               **{k: stats(v) for k, v in t.items()})
    med = lambda k: out[k]['median_ms']
    out['speedup'] = med('loop') / med('batch')
    out['speedup_1'] = med('loop_1') / med('batch_1')
    out['matching_share_before'] = med('loop') / med('chunk_before')
    out['matching_share_after'] = med('batch') / med('chunk_after')
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
