"""Float64 numpy restatement of N7 (include/buffer_hip.h: Fast Global Registration), the reference of tests/test_fgr_cpu.py and
tests/test_fgr_gpu.py.  The sampler is vectorised in np.uint64 arithmetic (all trials at once, then the first max_tuples accepted
ones); the optimisation uses plain numpy sums, so it differs from the device by the order of its sums only."""
import numpy as np

NOTHING, OK, FAILED = 0, 1, 2
MIN_ROWS = 10
_M64 = (1 << 64) - 1


def splitmix64(x):
    """the mixer of csrc/registration.hip on a Python int"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def splitmix64_np(x):
    """the same on an np.uint64 array (wrapping arithmetic)"""
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _edge2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def tuples(src, tgt, corr, seed, tuple_scale=0.95, max_tuples=1000, trial_factor=100):
    """-> (rows int32[3 * max_tuples, 2] with the tail -1, tuples kept, trials examined)"""
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    n = len(corr)
    rows = np.full((3 * max_tuples, 2), -1, np.int32)
    ntrial = trial_factor * n
    if n == 0:
        return rows, 0, 0
    s2 = float(tuple_scale) * float(tuple_scale)
    with np.errstate(over='ignore'):
        base = np.uint64(seed & _M64) + np.uint64(3) * np.arange(ntrial, dtype=np.uint64)
        r = np.stack([splitmix64_np(base + np.uint64(k)) % np.uint64(n) for k in range(3)], 1).astype(np.int64)     # [ntrial, 3]
    c = corr[r]                                                   # [ntrial, 3, 2]
    inside = ((c[..., 0] >= 0) & (c[..., 0] < len(src)) & (c[..., 1] >= 0) & (c[..., 1] < len(tgt))).all(1)
    cs = np.where(inside[:, None], c[..., 0], 0) if len(src) else np.zeros_like(c[..., 0])
    ct = np.where(inside[:, None], c[..., 1], 0) if len(tgt) else np.zeros_like(c[..., 1])
    if len(src) == 0 or len(tgt) == 0:
        return rows, 0, ntrial
    P, Q = src[cs].astype(np.float64), tgt[ct].astype(np.float64)  # [ntrial, 3, 3]
    ok = inside & np.isfinite(P).all((1, 2)) & np.isfinite(Q).all((1, 2))
    with np.errstate(invalid='ignore', over='ignore'):
        for i, j in ((0, 1), (1, 2), (2, 0)):
            a, b = _edge2(Q[:, i], Q[:, j]), _edge2(P[:, i], P[:, j])
            ok &= (s2 * a < b) & (s2 * b < a)
    acc = np.flatnonzero(ok)
    kept = min(len(acc), max_tuples)
    examined = int(acc[max_tuples - 1]) + 1 if len(acc) >= max_tuples else ntrial
    rows[:3 * kept] = c[acc[:kept]].reshape(-1, 2)
    return rows, kept, examined


def tuples_sequential(src, tgt, corr, seed, tuple_scale=0.95, max_tuples=1000, trial_factor=100):
    """the same list by a plain loop over the trials (what the vectorised sampler is pinned against)"""
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    n, out = len(corr), []
    s2 = float(tuple_scale) * float(tuple_scale)
    examined = trial_factor * n
    for t in range(trial_factor * n):
        r = [splitmix64((seed + 3 * t + k) & _M64) % n for k in range(3)]
        c = corr[r]
        if not all(0 <= int(a) < len(src) and 0 <= int(b) < len(tgt) for a, b in c):
            continue
        P, Q = src[c[:, 0]].astype(np.float64), tgt[c[:, 1]].astype(np.float64)
        if not (np.isfinite(P).all() and np.isfinite(Q).all()):
            continue
        good = True
        for i, j in ((0, 1), (1, 2), (2, 0)):
            a, b = float(_edge2(Q[i], Q[j])), float(_edge2(P[i], P[j]))
            good = good and s2 * a < b and s2 * b < a
        if good:
            out.append(c)
            if len(out) == max_tuples:
                examined = t + 1
                break
    rows = np.full((3 * max_tuples, 2), -1, np.int32)
    if out:
        rows[:3 * len(out)] = np.concatenate(out)
    return rows, len(out), examined


def normalisation(src, tgt):
    """-> (c_src, c_tgt, D) or None for an empty cloud / D == 0; non-finite rows are left out"""
    cs = []
    dmax = 0.0
    for p in (src, tgt):
        p = np.asarray(p, np.float32).reshape(-1, 3).astype(np.float64)
        p = p[np.isfinite(p).all(1)]
        if len(p) == 0:
            return None
        c = p.sum(0) / len(p)
        dmax = max(dmax, float(np.sqrt(_edge2(p, c)).max()))
        cs.append(c)
    if not dmax > 0.0:
        return None
    return cs[0], cs[1], dmax


def solve6(H, g):
    """H x = -g by LDL^T without pivoting (icp_solve6) -> x or None"""
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        d = H[j, j]
        for m in range(j):
            d -= L[j, m] * L[j, m] * D[m]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        D[j] = d
        for i in range(j + 1, 6):
            e = H[i, j]
            for m in range(j):
                e -= L[i, m] * L[j, m] * D[m]
            L[i, j] = e / d
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        e = -g[i]
        for m in range(i):
            e -= L[i, m] * y[m]
        y[i] = e
    for i in range(5, -1, -1):
        e = y[i] / D[i]
        for m in range(i + 1, 6):
            e -= L[m, i] * x[m]
        x[i] = e
    return x if np.isfinite(x).all() else None


def delta_transform(x):
    """[Rz(x2) Ry(x1) Rx(x0) | x3..5]"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = x[3:6]
    return T


def optimise(src, tgt, rows, kept, max_tuples, mu_start=1.0, delta=0.025, delta_absolute=0, division_factor=1.4, decrease_every=4,
             iterations=64):
    """-> (T f64[4,4], status, updates, weights f64[3 * max_tuples])"""
    weights = np.full(3 * max_tuples, np.nan)
    m = 3 * kept
    nrm = normalisation(src, tgt)
    if nrm is None or m < MIN_ROWS:
        return np.eye(4), NOTHING, 0, weights
    c_src, c_tgt, D = nrm
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    s = (src[rows[:m, 0]].astype(np.float64) - c_src) / D
    p = (tgt[rows[:m, 1]].astype(np.float64) - c_tgt) / D
    T, mu = np.eye(4), float(mu_start)
    floor = (delta / D) * (delta / D) if delta_absolute else float(delta)
    status, updates = OK, 0
    for it in range(iterations):
        q = s @ T[:3, :3].T + T[:3, 3]
        r = p - q
        rr = _edge2(r, np.zeros(3))
        with np.errstate(invalid='ignore', over='ignore'):
            w = np.where(np.isfinite(rr), (mu / (rr + mu)) ** 2, 0.0)
        weights[:m] = w
        J = np.zeros((m, 3, 6))                                   # the three Jacobian rows of every kept row
        J[:, 0, 1], J[:, 0, 2], J[:, 0, 3] = -q[:, 2], q[:, 1], -1.0
        J[:, 1, 0], J[:, 1, 2], J[:, 1, 4] = q[:, 2], -q[:, 0], -1.0
        J[:, 2, 0], J[:, 2, 1], J[:, 2, 5] = -q[:, 1], q[:, 0], -1.0
        use = w != 0.0
        H = np.einsum('n,nca,ncb->ab', w[use], J[use], J[use])
        g = np.einsum('n,nca,nc->a', w[use], J[use], r[use])
        x = solve6(H, g)
        if x is None:
            status = FAILED
            break
        T = delta_transform(x) @ T
        updates += 1
        if it % decrease_every == 0 and mu > floor:
            mu /= division_factor
    out = np.eye(4)
    if updates > 0:
        out[:3, :3] = T[:3, :3]
        out[:3, 3] = D * T[:3, 3] + c_tgt - T[:3, :3] @ c_src
    return out, status, updates, weights


def fgr(src, tgt, corr, seed, tuple_scale=0.95, max_tuples=1000, trial_factor=100, mu_start=1.0, delta=0.025, delta_absolute=0,
        division_factor=1.4, decrease_every=4, iterations=64):
    """one pair -> dict(T, info int32[4], rows, weights): buf_fgr_batched's outputs"""
    rows, kept, examined = tuples(src, tgt, corr, seed, tuple_scale, max_tuples, trial_factor)
    T, status, updates, weights = optimise(src, tgt, rows, kept, max_tuples, mu_start, delta, delta_absolute, division_factor,
                                           decrease_every, iterations)
    return dict(T=T, info=np.array([status, kept, examined, updates], np.int32), rows=rows, weights=weights)
