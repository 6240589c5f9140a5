"""The bits of the batched pose estimators on a fixed, seeded set of small cases: every output tensor of ops.icp_batched (three
methods), ops.vgicp_batched, ops.fgr_batched, ops.sc2_batched and ops.clique_batched as the sha256 of its raw bytes (NaN payloads
included), written to a JSON file.  BUF_LIB_PATH chooses the library, so two builds can be compared key for key:

    BUF_LIB_PATH=old.so python tools/estimator_bits.py --out old.json
    python tools/estimator_bits.py --out new.json

For a refactor that must not move a bit (profiles/pose_math_refactor.md); not a test: a deliberate change of the arithmetic, or a
compiler that orders it differently, changes the hashes.  The shapes are the smallest at which the shared routines take another path:
source lengths 0 / 1 / 255 / 256 / 257 / 700 in one batch (the 256-point tile seam: no, one, two and three records per pair), NaN
rows, a collinear pair (rank-1 H) and a planar one (rank 2), pairs with fewer than 3 / 6 matches, a pair that is still moving after
the 8th round (max_iteration=30: the probe readback is crossed; the iteration counts are in the file), and pairs of 0 / 2 / 3 / 64 /
65 / 300 correspondences of which some end NOTHING."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buffer_amd import ops  # noqa: E402


def surface(rng, n):
    """n points of a bumpy sheet over the unit square and their unit normals"""
    x, y = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    z = 0.2 * np.sin(3 * x) * np.cos(2 * y)
    nrm = np.stack([-0.6 * np.cos(3 * x) * np.cos(2 * y), 0.4 * np.sin(3 * x) * np.sin(2 * y), np.ones(n)], 1)
    return np.stack([x, y, z], 1), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def motion(rng, angle, shift):
    """a rigid motion of about `angle` radians and `shift` units, as a 4x4"""
    a = rng.standard_normal(3)
    a = a / np.linalg.norm(a) * angle
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.linalg.norm(a)
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.standard_normal(3) * shift / np.sqrt(3)
    return T


def icp_batch(rng):
    """(src, src normals, src lengths, tgt, tgt normals, tgt lengths, T_init) of the ICP / VGICP pairs"""
    S, SN, T, TN, sl, tl = [], [], [], [], [], []

    def pair(ns, nt=900, angle=0.03, shift=0.02, edit=None):
        t, tn = surface(rng, nt)
        M = motion(rng, angle, shift)
        k = rng.integers(0, nt, ns)
        s = (t[k] - M[:3, 3]) @ M[:3, :3] + rng.standard_normal((len(k), 3)) * 0.002      # M s = t
        sn = tn[k] @ M[:3, :3]
        if edit:
            s, sn, t, tn = edit(s, sn, t, tn)
        S.append(s); SN.append(sn); T.append(t); TN.append(tn); sl.append(len(s)); tl.append(len(t))

    for ns in (0, 1, 255, 256, 257, 700):
        pair(ns)

    def nan_rows(s, sn, t, tn):
        s[::7] = np.nan; s[3, 1] = np.inf; sn[5::11] = np.nan; sn[2] *= 1.01; t[::13, 2] = np.nan; tn[4::9] = 0.0
        return s, sn, t, tn
    pair(300, edit=nan_rows)

    def collinear(s, sn, t, tn):
        u = np.linspace(0, 1, len(t))[:, None] * np.array([[0.6, 0.8, 0.0]])
        return u[:len(s)] + 0.01, sn, u, tn
    pair(100, nt=200, edit=collinear)

    def planar(s, sn, t, tn):
        s[:, 2] = 0.01; t[:, 2] = 0.0; sn[:] = (0, 0, 1); tn[:] = (0, 0, 1)
        return s, sn, t, tn
    pair(200, edit=planar)

    def two_near(s, sn, t, tn):
        s[2:] += 50.0
        return s, sn, t, tn
    pair(5, edit=two_near)                              # 2 matches: below the 3 of Kabsch and the 6 of the 6x6 step
    pair(5)                                             # 5 matches: enough for Kabsch, too few for the 6x6 step
    pair(40, edit=lambda s, sn, t, tn: (s + 50.0, sn, t, tn))      # far from its target: no match
    pair(600, angle=0.25, shift=0.12)                   # far off: still moving after the 8th round
    pair(513, angle=0.15, shift=0.08)
    cat = lambda a: np.concatenate(a).astype(np.float32)
    return cat(S), cat(SN), sl, cat(T), cat(TN), tl, np.tile(np.eye(4), (len(sl), 1, 1))


def corr_batch(rng):
    """(src, src lengths, tgt, tgt lengths, corr, corr lengths) of the FGR / SC2 / clique pairs"""
    S, T, Cr, sl, tl, cl = [], [], [], [], [], []

    def pair(nc, inliers=0.6, npts=400, edit=None):
        s, _ = surface(rng, npts)
        s[:, 2] += rng.uniform(0, 0.5, npts)            # a volume, not a sheet
        M = motion(rng, 0.8, 0.5)
        t = s @ M[:3, :3].T + M[:3, 3] + rng.standard_normal((npts, 3)) * 0.005
        i = rng.integers(0, npts, nc)
        j = np.where(rng.uniform(0, 1, nc) < inliers, i, rng.integers(0, npts, nc))
        if edit:
            s, t = edit(s, t)
        S.append(s); T.append(t); Cr.append(np.stack([i, j], 1)); sl.append(npts); tl.append(npts); cl.append(nc)

    for nc in (0, 2, 3, 64, 65, 300):
        pair(nc)
    pair(120, inliers=0.0)                              # no consensus: NOTHING

    def nan_rows(s, t):
        s[::5] = np.nan; t[1::17, 0] = np.inf
        return s, t
    pair(200, edit=nan_rows)

    def collinear(s, t):
        u = np.linspace(0, 1, len(s))[:, None]
        return u * np.array([[0.6, 0.8, 0.0]]), u * np.array([[0.0, 0.6, 0.8]]) + 1.0
    pair(150, inliers=1.0, edit=collinear)

    def planar(s, t):
        s[:, 2] = 0.0
        M = motion(np.random.default_rng(5), 0.5, 0.3)
        return s, s @ M[:3, :3].T + M[:3, 3]
    pair(256, inliers=0.8, edit=planar)
    pair(257, inliers=0.3)
    bad = np.stack([rng.integers(-3, 500, 30), rng.integers(-3, 500, 30)], 1)      # indices outside the clouds: dead rows
    Cr[-1][:30] = bad
    return (np.concatenate(S).astype(np.float32), sl, np.concatenate(T).astype(np.float32), tl, np.concatenate(Cr).astype(np.int32), cl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out, notes = {}, {}

    def put(case, names, tensors):
        for name, t in zip(names, tensors):
            if isinstance(t, dict):
                put(case, [f'{name}.{k}' for k in t], t.values())
            elif t is not None:
                torch.cuda.synchronize()
                out[f'{case}/{name}'] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    src, snrm, sl, tgt, tnrm, tl, T0 = icp_batch(np.random.default_rng(11))
    d = lambda x, dt=torch.float32: torch.as_tensor(x, dtype=dt, device=dev)
    icp_names = ('T', 'fitness', 'rmse', 'iterations', 'nn')
    for method in ('point_to_point', 'point_to_plane', 'generalized'):
        for max_it in (30, 3, 0):
            r = ops.icp_batched(d(src), sl, d(tgt), tl, 0.15, d(T0, torch.float64), method=method, tgt_normals=d(tnrm), max_iteration=max_it,
                                correspondences=True, src_normals=d(snrm), epsilon=1e-3)
            put(f'icp {method} max_iteration={max_it}', icp_names, r)
            notes[f'icp {method} max_iteration={max_it}: iterations'] = r[3].cpu().tolist()
    vmap = ops.voxel_map_build(d(tgt), tl, 0.1, normals=d(tnrm), epsilon=1e-3)
    put('voxel map', ('rows',), (vmap.rows(),))
    for k in ops.VGICP_NEIGHBORS:
        for with_normals in (True, False):
            r = ops.vgicp_batched(d(src), sl, vmap, d(T0, torch.float64), neighbors=k, src_normals=d(snrm) if with_normals else None,
                                  max_iteration=30, rows=True)
            case = f'vgicp neighbors={k} {"with" if with_normals else "without"} source normals'
            put(case, icp_names[:4] + ('row',), r)
            notes[f'{case}: iterations'] = r[3].cpu().tolist()
    pc = [len(sl) - 1 - b for b in range(len(sl))]                 # every pair against another cloud of the map
    put('vgicp pair_cloud reversed', icp_names[:4] + ('row',),
        ops.vgicp_batched(d(src), sl, vmap, d(T0, torch.float64), neighbors=7, src_normals=d(snrm), pair_cloud=pc, max_iteration=5, rows=True))

    cs, csl, ct, ctl, corr, ccl = corr_batch(np.random.default_rng(12))
    corr_d = torch.as_tensor(corr, dtype=torch.int32, device=dev)
    r = ops.fgr_batched(d(cs), csl, d(ct), ctl, corr_d, ccl, return_rows=True)
    put('fgr', ('T', 'info', 'rows', 'weights'), r)
    notes['fgr: info'] = r[1].cpu().tolist()
    put('fgr max_tuples=50 iterations=7 absolute delta', ('T', 'info', 'rows', 'weights'),
        ops.fgr_batched(d(cs), csl, d(ct), ctl, corr_d, ccl, seeds=range(100, 100 + len(ccl)), max_tuples=50, delta=0.01, delta_absolute=True,
                        iterations=7, return_rows=True))
    r = ops.sc2_batched(d(cs), csl, d(ct), ctl, corr_d, ccl, 0.05, 0.05, return_detail=True)
    put('sc2', ('T', 'info', 'detail'), r)
    notes['sc2: info'] = r[1].cpu().tolist()
    put('sc2 nms max_seeds=16 k1=5 refine_iterations=1', ('T', 'info', 'detail'),
        ops.sc2_batched(d(cs), csl, d(ct), ctl, corr_d, ccl, 0.05, 0.08, seed_ratio=1.0, max_seeds=16, k1=5, nms_radius=0.05,
                        power_iterations=3, refine_iterations=1, return_detail=True))
    r = ops.clique_batched(d(cs), csl, d(ct), ctl, corr_d, ccl, 0.05, return_detail=True)
    put('clique', ('T', 'info', 'detail'), r)
    notes['clique: info'] = r[1].cpu().tolist()
    put('clique max_seeds=8 max_members=16 refine_iterations=0', ('T', 'info', 'detail'),
        ops.clique_batched(d(cs), csl, d(ct), ctl, corr_d, ccl, 0.05, max_seeds=8, max_members=16, gnc_iterations=5, refine_iterations=0,
                           return_detail=True))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'sha256': out, 'notes': notes}, f, indent=1, sort_keys=True)
    print(f'{len(out)} tensors -> {a.out}')


if __name__ == '__main__':
    main()
