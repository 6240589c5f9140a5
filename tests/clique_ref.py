"""Float64 numpy restatement of N10 (include/buffer_hip.h: compatibility graph, core numbers, greedy cliques, GNC-TLS rotation over
the translation-invariant measurements, component-wise TLS voting, N8's refinement), the reference of tests/test_clique_cpu.py and
tests/test_clique_gpu.py.  Written from the specification, not from the kernels: a dense boolean matrix (no bit rows), a sequential
peel by smallest degree, numpy's SVD and numpy's sums.  The decisions follow the specification literally; float sums run in numpy's
order.

clique(...) also returns the margins of every decision that the GPU tests compare exactly."""
import math

import numpy as np

import sc2_ref

NOTHING, OK = 0, 1
DEFAULTS = dict(max_seeds=64, max_members=256, gnc_factor=1.4, gnc_iterations=100, refine_iterations=20)


def core_numbers(C, live):
    """C bool[n,n] (symmetric, zero diagonal, zero on dead rows) -> int[n]: the core number of every live row, -1 on dead rows.
    Peeling by smallest remaining degree: the core number of the vertex removed is the largest smallest-degree seen so far."""
    n = len(C)
    deg = C.sum(1).astype(np.int64)
    core = np.full(n, -1, np.int64)
    alive = live.copy()
    k = 0
    big = n + 1
    work = np.where(alive, deg, big)
    for _ in range(int(live.sum())):
        v = int(np.argmin(work))
        k = max(k, int(work[v]))
        core[v] = k
        alive[v] = False
        work[v] = big
        work[C[v] & alive] -= 1
    return core


def rotation_of(H):
    """R = V diag(1, 1, det(V U^T)) U^T of H = U S V^T; the identity for H = 0 or a non-finite H"""
    R = np.eye(3)
    if np.isfinite(H).all() and np.abs(H).max() > 0:
        U, _, Vt = np.linalg.svd(H)
        R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return R


def rotate(R, P):
    """R p of every row as ((R0 px + R1 py) + R2 pz)"""
    return np.stack([(R[k, 0] * P[:, 0] + R[k, 1] * P[:, 1]) + R[k, 2] * P[:, 2] for k in range(3)], 1)


def gnc_rotation(Pm, Qm, tim_thr, gnc_factor, gnc_iterations, margins):
    """the members' points (walk order) -> (R, weights f64[M], steps)"""
    K = len(Pm)
    a, b = np.triu_indices(K, 1)                                 # a < b, lexicographic
    alpha, beta = Pm[b] - Pm[a], Qm[b] - Qm[a]
    M = len(a)
    c2 = tim_thr * tim_thr
    w = np.ones(M)
    prev = (0, M)
    mu = None
    steps = 0
    R = np.eye(3)
    for it in range(gnc_iterations):
        steps = it + 1
        H = (w[:, None] * alpha).T @ beta
        R = rotation_of(H)
        d = beta - rotate(R, alpha)
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        if it == 0:
            g = 2.0 * r2.max() / c2 - 1.0
            margins['g'] = min(margins['g'], abs(g))
            if g <= 0:
                w = np.ones(M)
                break
            mu = 1.0 / g
        hi, lo = ((mu + 1.0) / mu) * c2, (mu / (mu + 1.0)) * c2
        margins['gnc'] = min(margins['gnc'], float(np.abs(r2 - hi).min() / c2), float(np.abs(r2 - lo).min() / c2))
        mid = np.sqrt((c2 * (mu * (mu + 1.0))) / np.where(r2 > 0, r2, 1.0)) - mu
        w = np.where(r2 >= hi, 0.0, np.where(r2 <= lo, 1.0, mid))
        now = (int((w == 0.0).sum()), int((w == 1.0).sum()))
        if (it >= 1 and now[0] + now[1] == M and now == prev) or it + 1 == gnc_iterations:
            break
        prev = now
        mu = mu * gnc_factor
    return R, w, steps


def vote(v, c, margins):
    """component-wise TLS voting over the values v (member order) -> the estimate"""
    K = len(v)
    e = np.sort(np.concatenate([v - c, v + c]))
    h = (e[:-1] + e[1:]) * 0.5
    dist = np.abs(v[None, :] - h[:, None])                       # [2K - 1, K]
    # An exact tie is left out of the margin: two equal endpoints (repeated rows) give a candidate ON the endpoint, at distance c from
    # the values that made it.  Whichever way that comparison rounds, the candidate's consensus set is that of the interval to its
    # left or to its right, whose estimate (the same members summed in the same order) is the same bits: the result cannot depend on it.
    own = (e[:-1] == e[1:])[:, None] & (((v - c)[None, :] == h[:, None]) | ((v + c)[None, :] == h[:, None]))
    if (~own).any():
        margins['vote'] = min(margins['vote'], float(np.abs(dist - c)[~own].min()))
    inside = dist <= c
    cnt = inside.sum(1)
    best, best_cost, best_set, costs = None, math.inf, None, []
    for j in range(len(h)):
        if cnt[j] == 0:
            continue
        vs = v[inside[j]]
        est = vs.sum() / cnt[j]
        cost = ((vs - est) * (vs - est)).sum() + (K - cnt[j]) * (c * c)
        costs.append((cost, inside[j].tobytes()))
        if cost < best_cost:
            best, best_cost, best_set = est, cost, inside[j].tobytes()
    other = [cost for cost, s in costs if s != best_set]         # (candidates with the winner's consensus set tie exactly)
    if other:
        margins['vote_gap'] = min(margins['vote_gap'], float(min(other) - best_cost))
    return 0.0 if best is None else float(best)


def clique(src, tgt, corr, d_thr, tim_thr=None, t_thr=None, inlier_thr=None, max_seeds=64, max_members=256, gnc_factor=1.4,
           gnc_iterations=100, refine_iterations=20):
    """one pair -> dict(T f64[4,4], info int32[8], deg / core / rank int32[n], sizes int32[max_seeds], members int32[max_members],
    weights f64[max_members (max_members - 1) / 2] (NaN tail), pose0 f64[12], inliers uint8[n], certified bool, peel_levels int,
    margins dict(compat, gnc, g, vote, vote_gap, residual))."""
    tim_thr = d_thr if tim_thr is None else tim_thr
    t_thr = d_thr / 2 if t_thr is None else t_thr
    inlier_thr = d_thr if inlier_thr is None else inlier_thr
    P, Q, live = sc2_ref.rows_of(src, tgt, corr)
    n = len(P)
    both = live[:, None] & live[None, :]
    e = np.abs(sc2_ref.distances(P) - sc2_ref.distances(Q))
    C = (e <= d_thr) & both
    np.fill_diagonal(C, False)
    offdiag = both & ~np.eye(n, dtype=bool)
    margins = dict(compat=float(np.abs(e - d_thr)[offdiag].min()) if offdiag.any() else math.inf, gnc=math.inf, g=math.inf, vote=math.inf,
                   vote_gap=math.inf, residual=math.inf)
    n_live = int(live.sum())
    deg = np.where(live, C.sum(1), -1).astype(np.int32)
    core = core_numbers(C, live).astype(np.int32)
    bound = int(core.max()) + 1 if n_live else 0
    order = sorted(np.flatnonzero(live).tolist(), key=lambda i: (-core[i], -deg[i], i))
    rank = np.full(n, -1, np.int32)
    rank[order] = np.arange(len(order))

    # the walks, in rank space: the first set bit of the candidates is the candidate of lowest rank
    Cr = C[np.ix_(order, order)]
    S = min(max_seeds, n_live)
    sizes = np.full(max_seeds, -1, np.int32)
    walks = []
    for r in range(S):
        cand = Cr[r].copy()
        walk = [r]
        while cand.any():
            j = int(np.argmax(cand))
            walk.append(j)
            cand &= Cr[j]
        walks.append(walk)
        sizes[r] = len(walk)
    win = max(range(S), key=lambda r: (sizes[r], -r)) if S else -1
    size = int(sizes[win]) if S else 0
    K = min(size, max_members)
    members = np.full(max_members, -1, np.int32)
    if S:
        members[:K] = [order[j] for j in walks[win][:K]]
    Mmax = max_members * (max_members - 1) // 2
    weights = np.full(Mmax, np.nan)
    pose0 = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
    T, inl = np.eye(4), np.zeros(n, bool)
    info = np.array([NOTHING, n_live, bound, size, win, K, 0, 0], np.int32)

    def score(R, t):
        r = sc2_ref.residuals(R, t, P, Q)
        if live.any():
            margins['residual'] = min(margins['residual'], float(np.abs(r[live] - inlier_thr).min()))
        return live & (r < inlier_thr)

    if size >= 3:
        m = members[:K]
        R, w, steps = gnc_rotation(P[m], Q[m], tim_thr, gnc_factor, gnc_iterations, margins)
        weights[:len(w)] = w
        x = Q[m] - rotate(R, P[m])
        t = np.array([vote(x[:, k].copy(), t_thr, margins) for k in range(3)])
        pose0 = np.concatenate([R.reshape(9), t])
        info[6] = steps
        last = 0
        for it in range(refine_iterations):
            now = score(R, t)
            if (it > 0 and now.sum() <= last) or now.sum() < 3:
                break
            last = int(now.sum())
            R, t = sc2_ref._mean_kabsch(P[now], Q[now])
        fin = score(R, t)
        if fin.sum() >= 3:
            inl = fin
            T[:3, :3], T[:3, 3] = R, t
            info[0], info[7] = OK, int(fin.sum())
    return dict(T=T, info=info, deg=deg, core=core, rank=rank, sizes=sizes, members=members, weights=weights, pose0=pose0,
                inliers=inl.astype(np.uint8), certified=bool(info[0] == OK and size == bound), peel_levels=len(set(core[live].tolist())),
                margins=margins)
