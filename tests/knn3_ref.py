"""The plain references of the k-NN search (N14) and of the statistical outlier rule (N15), written from the contract in
include/buffer_hip.h.  No grid, no rings, no early exit: every query meets every support of its element.

    d2 = (dx*dx + dy*dy) + dz*dz in float32, one rounding per operation (sqdist3); a pair whose d2 is not finite matches nothing;
    a row = the k smallest 64-bit keys (bits of d2) << 32 | global support index, ascending, padded with ns / +inf.

    mean_i = (sum in column order, float64, of sqrt(float64(d2_ij)) over the finite entries) / their number, -1 for an empty row;
    V = rows with entries, mu = sum(mean_i > 0) / V, sd = sqrt(sum_{mean_i > 0} (mean_i - mu)^2 / (V - 1)), thr = mu + ratio * sd;
    keep_i = mean_i > 0 and mean_i < thr.
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def sqdist3(q, s):
    """float32 [nq,ns] distances in the kernel's operation order"""
    q, s = np.asarray(q, np.float32).reshape(-1, 3), np.asarray(s, np.float32).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        dx = q[:, None, 0] - s[None, :, 0]
        dy = q[:, None, 1] - s[None, :, 1]
        dz = q[:, None, 2] - s[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def brute_force(queries, supports, q_lens, s_lens, k):
    """-> (nbr int32[nq,k] padded with ns, d2 float32[nq,k] padded with +inf)"""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(supports, np.float32).reshape(-1, 3)
    q_lens, s_lens = np.asarray(q_lens, np.int64), np.asarray(s_lens, np.int64)
    assert q_lens.sum() == len(q) and s_lens.sum() == len(s) and len(q_lens) == len(s_lens)
    nq, ns = len(q), len(s)
    nbr = np.full((nq, k), ns, np.int32)
    out = np.full((nq, k), np.inf, np.float32)
    q0 = s0 = 0
    for nqb, nsb in zip(q_lens, s_lens):
        if nqb and nsb:
            d2 = sqdist3(q[q0:q0 + nqb], s[s0:s0 + nsb])
            keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.arange(s0, s0 + nsb, dtype=np.uint64))[None, :]
            keys = np.where(np.isfinite(d2), keys, EMPTY)
            keys = np.sort(keys, axis=1)[:, :k]
            w = keys.shape[1]
            ok = keys != EMPTY
            nbr[q0:q0 + nqb, :w] = np.where(ok, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), ns).astype(np.int32)
            out[q0:q0 + nqb, :w] = np.where(ok, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
        q0 += nqb
        s0 += nsb
    return nbr, out


def d2_of(queries, supports, nbr):
    """sqdist3 of every reported index (float32[nq,k]), +inf where the entry is padding"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    s = np.asarray(supports, np.float32).reshape(-1, 3)
    ns = len(s)
    pad = nbr >= ns
    sel = s[np.where(pad, 0, nbr)] if ns else np.zeros(nbr.shape + (3,), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = q[:, None, 0] - sel[..., 0], q[:, None, 1] - sel[..., 1], q[:, None, 2] - sel[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    return np.where(pad, np.float32(np.inf), d2).astype(np.float32)


def statistical(d2, lengths, std_ratio):
    """d2 float32[n,k] k-NN rows -> (mean float64[n], stats float64[nc,3] = mu, sd, thr, keep bool[n])"""
    d2 = np.asarray(d2, np.float32)
    n, k = d2.shape
    mean = np.full(n, -1.0, np.float64)
    for i in range(n):
        s, c = np.float64(0.0), 0
        for j in range(k):
            if not np.isfinite(d2[i, j]):
                break
            s = s + np.sqrt(np.float64(d2[i, j]))
            c += 1
        if c:
            mean[i] = s / np.float64(c)
    stats = np.zeros((len(lengths), 3), np.float64)
    keep = np.zeros(n, bool)
    lo = 0
    with np.errstate(invalid='ignore', divide='ignore'):
        for c, m in enumerate(lengths):
            mi = mean[lo:lo + m]
            V = np.float64((mi >= 0).sum())
            pos = mi[mi > 0]
            mu = np.float64(pos.sum()) / V
            sd = np.sqrt(np.float64(((pos - mu) ** 2).sum()) / (V - np.float64(1.0)))
            thr = mu + np.float64(std_ratio) * sd
            stats[c] = mu, sd, thr
            keep[lo:lo + m] = (mi > 0) & (mi < thr)
            lo += m
    return mean, stats, keep
