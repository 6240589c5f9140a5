"""Float64 numpy restatement of N8 (include/buffer_hip.h: SC2-PCR, single stage), the reference of tests/test_sc2_cpu.py and
tests/test_sc2_gpu.py.  Written from the specification, not from the kernels: dense n x n matrices (no bit rows, no tiles), numpy's
SVD for the Kabsch step, and plain loops.  The two sums whose order the specification fixes (v_i = sum over ascending j, in the
confidence and in a set's weights) run column by column, which is that order for every row at once.

sc2(...) also returns the margins of every decision that the GPU tests compare exactly (the conditions of tests/test_sc2_cpu.py)."""
import math

import numpy as np

NOTHING, OK = 0, 1
DEFAULTS = dict(seed_ratio=0.2, max_seeds=512, k1=30, nms_radius=0.0, power_iterations=10, refine_iterations=20)


def rows_of(src, tgt, corr):
    """-> (P f64[n,3], Q f64[n,3], live bool[n]): the promoted points of every row, zeros on dead rows"""
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    n = len(corr)
    P, Q, live = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, bool)
    for i, (a, b) in enumerate(corr):
        if 0 <= a < len(src) and 0 <= b < len(tgt):
            p, q = src[a].astype(np.float64), tgt[b].astype(np.float64)
            if np.isfinite(p).all() and np.isfinite(q).all():
                P[i], Q[i], live[i] = p, q, True
    return P, Q, live


def distances(A):
    """d(a_i, a_j) for all pairs, in the written order"""
    dx, dy, dz = (A[:, None, k] - A[None, :, k] for k in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def power(S, start, iterations):
    """v <- S v (ascending j), v <- v / max v, `iterations` times"""
    v = start.astype(np.float64).copy()
    for _ in range(iterations):
        acc = np.zeros(len(v))
        for j in range(len(v)):
            acc = acc + S[:, j] * v[j]
        v = acc / acc.max() if len(acc) and acc.max() > 0 else acc
    return v


def kabsch(P, Q, u):
    """weights u (summing to 1) -> (R, t); the identity rotation for H = 0"""
    cp, cq = (u[:, None] * P).sum(0), (u[:, None] * Q).sum(0)
    H = np.zeros((3, 3))
    for i in range(len(P)):
        H += u[i] * np.outer(P[i] - cp, Q[i] - cq)
    R = np.eye(3)
    if np.isfinite(H).all() and np.abs(H).max() > 0:
        U, _, Vt = np.linalg.svd(H)
        R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return R, cq - R @ cp


def residuals(R, t, P, Q):
    r = np.stack([(((R[k, 0] * P[:, 0] + R[k, 1] * P[:, 1]) + R[k, 2] * P[:, 2]) + t[k]) - Q[:, k] for k in range(3)], 1)
    return np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])


def sc2(src, tgt, corr, d_thr, inlier_thr, seed_ratio=0.2, max_seeds=512, k1=30, nms_radius=0.0, power_iterations=10,
        refine_iterations=20):
    """one pair -> dict(T f64[4,4], info int32[6], conf f64[n] (NaN on dead rows), seeds int32[max_seeds], hyp_counts
    int32[max_seeds], counts int32[max_seeds, n], inliers uint8[n], margins dict(compat, residual, seed, nms)).
    margins: the smallest |e_ij - d_thr| over live pairs, | |R p + t - q| - inlier_thr | over every pose scored, and confidence gap
    over the comparisons that place a seed (the cut included) and over the suppression's comparisons.  An exact tie is left out of
    the gaps: the specification decides it by the row number, and it is a tie for whoever follows the fixed order of the sums (the
    ties that occur are repeated rows and the two symmetric rows of n = 2)."""
    P, Q, live = rows_of(src, tgt, corr)
    n = len(P)
    both = live[:, None] & live[None, :]
    dP = distances(P)
    e = np.abs(dP - distances(Q))
    C = (e <= d_thr) & both
    S = np.where(both, np.maximum(0.0, 1.0 - (e * e) / (d_thr * d_thr)), 0.0)
    margins = dict(compat=float(np.abs(e - d_thr)[both].min()) if both.any() else math.inf, residual=math.inf, seed=math.inf, nms=math.inf)

    v = power(S, live, power_iterations)
    conf = np.where(live, v, np.nan)
    c = np.where(live, v, -1.0)
    if nms_radius > 0:
        for i in np.flatnonzero(live):
            near = live & (dP[i] <= nms_radius)
            near[i] = False
            if near.any():
                gap = np.abs(v[near] - v[i])
                if (gap > 0).any():                              # (an exact tie is no comparison of roundings: see sc2's docstring)
                    margins['nms'] = min(margins['nms'], float(gap[gap > 0].min()))
                if (v[near] > v[i]).any():
                    c[i] = -1.0
    n_seed = min(max_seeds, max(1, math.ceil(seed_ratio * n)))
    order = sorted(range(n), key=lambda i: (-c[i], i))
    for a, b in zip(order[:n_seed], order[1:n_seed + 1]):        # every comparison that places a seed, the cut included
        if c[a] > 0 and c[a] != c[b]:
            margins['seed'] = min(margins['seed'], float(c[a] - max(c[b], 0.0)))
    seed_rows = [i for i in order[:n_seed] if c[i] > 0]

    seeds, hyp_counts = np.full(max_seeds, -1, np.int32), np.full(max_seeds, -1, np.int32)
    counts = np.full((max_seeds, n), -1, np.int32)
    Cf = C.astype(np.float64)                                    # (0 / 1 products and sums below 2^53: exact in float64)
    second = (Cf[seed_rows] @ Cf).astype(np.int64) if seed_rows else np.zeros((0, n), np.int64)
    poses = {}

    def score(R, t):
        r = residuals(R, t, P, Q)
        if live.any():
            margins['residual'] = min(margins['residual'], float(np.abs(r[live] - inlier_thr).min()))
        return live & (r < inlier_thr)

    for rank, s in enumerate(seed_rows):
        seeds[rank] = s
        K = C[s].astype(np.int64) * second[rank]
        counts[rank] = K
        members = [j for j in sorted(range(n), key=lambda j: (-K[j], j))[:k1] if K[j] > 0]
        if len(members) < 3:
            continue
        w = power(S[np.ix_(members, members)], np.ones(len(members)), power_iterations)
        R, t = kabsch(P[members], Q[members], w / w.sum())
        poses[rank] = (R, t)
        hyp_counts[rank] = int(score(R, t).sum())

    T, inl = np.eye(4), np.zeros(n, bool)
    info = np.array([NOTHING, int(live.sum()), len(seed_rows), -1, 0, 0], np.int32)
    if poses:
        win = max(poses, key=lambda r: (hyp_counts[r], -r))
        info[3], info[4] = seeds[win], hyp_counts[win]
        if live.sum() >= 3 and hyp_counts[win] >= 3:
            R, t = poses[win]
            last = 0
            for it in range(refine_iterations):
                now = score(R, t)
                if (it > 0 and now.sum() <= last) or now.sum() < 3:
                    break
                last = int(now.sum())
                R, t = _mean_kabsch(P[now], Q[now])
            inl = score(R, t)
            T[:3, :3], T[:3, 3] = R, t
            info[0], info[5] = OK, int(inl.sum())
    return dict(T=T, info=info, conf=conf, seeds=seeds, hyp_counts=hyp_counts, counts=counts, inliers=inl.astype(np.uint8), margins=margins)


def _mean_kabsch(P, Q):
    """the unweighted step of the refinement: means as sum / count, H as the plain sum"""
    cp, cq = P.sum(0) / len(P), Q.sum(0) / len(Q)
    H = (P - cp).T @ (Q - cq)
    R = np.eye(3)
    if np.isfinite(H).all() and np.abs(H).max() > 0:
        U, _, Vt = np.linalg.svd(H)
        R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return R, cq - R @ cp
