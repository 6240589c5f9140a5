"""TEST INFRASTRUCTURE: float64 restatement of the ISS keypoint contract of include/buffer_hip.h (N11), in numpy.  Every sum runs
over the row's columns in column order (one numpy operation per column, over all points at once: elementwise fp64, nothing fused);
the eigenvalues come from numpy.linalg.eigvalsh.  tests/test_iss_cpu.py pins it on hand cases; the GPU tests compare
buf_iss_keypoints with it.

    radius_rows(pts, radius, k, lengths)   the neighbour rows buf_grid_query gives (fp32 d2, ascending by (d2, index), padded with n);
                                           k=None: as many columns as the longest row holds
    iss(pts, nbr_sal, nbr_nms, ...)        -> dict(mask u8[n], saliency f64[n], eig f64[n,3] descending, undecided bool[n])

Undecided points, at MARGIN = 1e-9: a decision of the contract that rounding in the eigenvalues could turn.  Point i is undecided if
one of |l2 - g21 l1|, |l3 - g32 l2|, |l3| is below MARGIN * l1 (its own saliency hangs on a comparison that close), if a point of
its non-max row is undecided in that sense (the row's maximum hangs on it), or if an unequal s_j of that row lies within
MARGIN * max(l1_i, l1_j) of s_i.  Two points with the same neighbour set add it in different orders, so their saliencies differ in the
last bits: such points are real, the comparison leaves them out.
`chance_ties` marks what that rule cannot see: a point with s_i > 0 whose non-max row holds an s_j EQUAL to s_i although the two
covariances differ in some bit -- LAPACK happened to round both l3 to the same number, another solver need not (a true tie, as
between doubled points, has equal covariances).  The undecided set is as the contract's tests state it and does not include them; a
test that picks its own input asserts that it has none.
"""
import numpy as np

MARGIN = 1e-9


def radius_rows(pts, radius, k=None, lengths=None):
    """int32[n,k]: per point the <= k nearest points of its own cloud with fp32 d2 = (dx*dx + dy*dy) + dz*dz < radius^2 (fp32),
    itself included, ascending by (d2, index), padded with n.  A NaN or infinite point has an empty row and is in no row."""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    n = len(p)
    lens = [n] if lengths is None else list(lengths)
    r2 = np.float32(radius) * np.float32(radius)
    rows, lo = [], 0
    for m in lens:
        q = p[lo:lo + m]
        with np.errstate(invalid='ignore', over='ignore'):
            d = q[:, None, :] - q[None, :, :]
            sq = d * d
            d2 = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)
        for i in range(m):
            hit = np.flatnonzero(d2[i] < r2)
            rows.append(hit[np.lexsort((hit, d2[i][hit]))] + lo)
        lo += m
    if k is None:
        k = max([len(r) for r in rows] + [1])
    out = np.full((n, k), n, np.int32)
    for i, r in enumerate(rows):
        out[i, :min(len(r), k)] = r[:k]
    return out


def _columns(nbr, n, max_nn):
    nbr = np.asarray(nbr).reshape(n, -1) if n else np.zeros((0, 1), np.int64)
    k = nbr.shape[1]
    kmax = k if not max_nn else min(int(max_nn), k)
    nbr = nbr[:, :kmax].astype(np.int64)
    return nbr, (nbr >= 0) & (nbr < n)


def covariance(pts, nbr, max_nn=0):
    """-> (m int64[n], C f64[n,6] = (c00, c01, c02, c11, c12, c22), zero rows where m == 0): the contract's sums, in column order"""
    P = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(P)
    nbr, valid = _columns(nbr, n, max_nn)
    m = valid.sum(1)
    S = np.zeros((n, 3))
    for c in range(nbr.shape[1]):
        v = valid[:, c]
        S[v] = S[v] + P[nbr[v, c]]
    dm = np.maximum(m, 1).astype(np.float64)
    mu = S / dm[:, None]
    C = np.zeros((n, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for c in range(nbr.shape[1]):
        v = valid[:, c]
        d = P[nbr[v, c]] - mu[v]
        for e, (a, b) in enumerate(pairs):
            C[v, e] = C[v, e] + d[:, a] * d[:, b]
    return m, C / dm[:, None]


def eigenvalues(C):
    """C f64[n,6] -> f64[n,3] descending (LAPACK eigvalsh)"""
    C = np.asarray(C, np.float64).reshape(-1, 6)
    M = np.empty((len(C), 3, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = (C[:, e] for e in range(6))
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    return np.linalg.eigvalsh(M)[:, ::-1] if len(C) else np.zeros((0, 3))


def saliency_of(eig, g21, g32):
    """the contract's three conditions on eigenvalues f64[n,3] -> s f64[n]"""
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    ok = (l1 > 0) & (l2 < g21 * l1) & (l3 < g32 * l2)
    return np.where(ok, l3, 0.0)


def iss(pts, nbr_sal, nbr_nms, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, max_nn=0):
    n = len(np.asarray(pts).reshape(-1, 3))
    m, C = covariance(pts, nbr_sal, max_nn)
    eig = eigenvalues(C)
    eig[m < min_neighbors] = 0.0
    sal = saliency_of(eig, gamma_21, gamma_32)
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    live = m >= min_neighbors
    own = live & (l1 > 0) & ((np.abs(l2 - gamma_21 * l1) < MARGIN * l1) | (np.abs(l3 - gamma_32 * l2) < MARGIN * l1) |
                             (np.abs(l3) < MARGIN * l1))
    nb, valid = _columns(nbr_nms, n, max_nn)
    mask = np.zeros(n, np.uint8)
    undecided = own.copy()
    chance = np.zeros(n, bool)
    for i in range(n):
        js = nb[i][valid[i]]
        chance[i] = sal[i] > 0 and ((sal[js] == sal[i]) & (C[js] != C[i]).any(1)).any()
        if own[js].any():
            undecided[i] = True
        sj = sal[js]
        close = (sj != sal[i]) & (np.abs(sj - sal[i]) < MARGIN * np.maximum(l1[i], l1[js]))
        if close.any():
            undecided[i] = True
        mask[i] = sal[i] > 0 and len(js) >= min_neighbors and not (sj > sal[i]).any()
    return dict(mask=mask, saliency=sal, eig=eig, undecided=undecided, m=m, chance_ties=chance)
