"""numpy restatement of buf_pair_stats (csrc/pairstats.hip) for the tests of buffer_amd/pairs.py: the fp32 operations of the search in
the kernel's order, so that matches and nearest rows are EQUAL to the device's, and fp64 sums that differ from the device's by
summation order only.

Large pairs (more than 4e8 source x target rows) use scipy.spatial.cKDTree to propose candidates (the fp32 decision is then redone on
them); where scipy is absent they take the chunked brute force as well, which gives the same rows and is only slower."""
import numpy as np

U = 2.0 ** -53


def transform(src, T):
    """p = T s in fp64 with the association ((T0*sx + T1*sy) + T2*sz) + T3 -> f64[n,3]"""
    s = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    with np.errstate(all='ignore'):
        return np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1)


def _d2(q, t):
    """fp32 (dx*dx + dy*dy) + dz*dz of q f32[a,1,3] against t f32[1,b,3] (or matching shapes)"""
    with np.errstate(all='ignore'):
        d = q - t
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(src, tgt, T, radius, chunk=None):
    """-> (nn int32[n]: row of tgt or -1, p f64[n,3] the unrounded transformed source).  Strict d2 < r2 with r2 = r*r in fp32, ties
    to the smaller row (argmin returns the first minimum), rows whose fp32 search point is not finite skipped."""
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    p = transform(src, T)
    with np.errstate(all='ignore'):
        q = p.astype(np.float32)
    n, m = q.shape[0], tgt.shape[0]
    nn = np.full(n, -1, np.int32)
    if n == 0 or m == 0:
        return nn, p
    finite = np.isfinite(q).all(1)
    r2 = np.float32(radius) * np.float32(radius)
    rows = np.flatnonzero(finite)
    brute = rows
    if n * m > 4e8 and _have_scipy():
        brute = _nearest_tree(q, tgt, rows, radius, r2, nn)
    step = chunk or max(1, int(2e7 // max(m, 1)))
    for lo in range(0, brute.size, step):
        r = brute[lo:lo + step]
        d2 = _d2(q[r][:, None, :], tgt[None, :, :])
        d2 = np.where(d2 < r2, d2, np.float32(np.inf))
        j = np.argmin(d2, axis=1)
        hit = d2[np.arange(r.size), j] < np.float32(np.inf)
        nn[r[hit]] = j[hit]
    return nn, p


def _have_scipy():
    try:
        import scipy.spatial  # noqa: F401
        return True
    except ImportError:
        return False


def _nearest_tree(q, tgt, rows, radius, r2, nn, K=16):
    """large clouds: a KD-tree proposes the K nearest targets within 1.01 r (fp64), the fp32 decision is redone on those; a row
    whose K-th candidate is not clearly farther than its first is handed back for brute force.  -> rows left for brute force"""
    from scipy.spatial import cKDTree
    ok = np.isfinite(tgt).all(1)
    keep = np.flatnonzero(ok)
    tree = cKDTree(tgt[keep].astype(np.float64))
    dist, idx = tree.query(q[rows].astype(np.float64), k=K, distance_upper_bound=1.01 * float(radius))
    full = np.isfinite(dist[:, K - 1]) & ~(dist[:, K - 1] > dist[:, 0] * (1 + 1e-4) + 1e-30)
    cand = np.where(np.isfinite(dist), idx, 0)
    c = keep[np.minimum(cand, keep.size - 1)]
    d2 = _d2(q[rows][:, None, :], tgt[c])
    d2 = np.where(np.isfinite(dist) & (d2 < r2), d2, np.float32(np.inf))
    # ties to the smaller ROW (not the smaller tree rank): lexicographic minimum of (d2, row)
    best = d2.min(axis=1)
    row = np.where(d2 == best[:, None], c, np.iinfo(np.int64).max).min(axis=1)
    hit = (best < np.float32(np.inf)) & ~full
    nn[rows[hit]] = row[hit]
    return rows[full]


def pair_ref(src, tgt, T, radius):
    """-> dict(n_src, matched, nn, terms f64[matched,10]: per match d2, u (3), upper triangle of u u^T (6), matched_pts f64[matched,3])"""
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    nn, p = nearest(src, tgt, T, radius)
    hit = np.flatnonzero(nn >= 0)
    u = tgt[nn[hit]].astype(np.float64)
    d = p[hit] - u
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    terms = np.stack([d2, u[:, 0], u[:, 1], u[:, 2], u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1],
                      u[:, 1] * u[:, 2], u[:, 2] * u[:, 2]], 1).reshape(-1, 10)
    return dict(n_src=int(nn.shape[0]), matched=int(hit.size), nn=nn, terms=terms, matched_pts=u)


def sum_bound(terms):
    """two fp64 sums of the same n terms in different orders differ by at most 2 (n - 1) 2^-53 sum|term| (to first order; each
    side's error is (n - 1) u sum|term|) -> bound per column of terms[n, k]"""
    t = np.asarray(terms, np.float64)
    return 2.0 * max(t.shape[0] - 1, 0) * U * np.abs(t).sum(0)


def check_moments(got, ref):
    """got: moments f64[10] of the device (sum_d2, sum_u, sum_uu); ref: pair_ref(...)"""
    want = ref['terms'].sum(0) if ref['matched'] else np.zeros(10)
    bound = sum_bound(ref['terms']) if ref['matched'] else np.zeros(10)
    diff = np.abs(np.asarray(got, np.float64).reshape(10) - want)
    assert np.all(diff <= bound), f'moments differ beyond the summation bound: diff={diff} bound={bound}'


def info_bound(points):
    """entry-wise summation bound of the 3DMatch-convention information matrix of `points` (synth.information_matrix: sum over the points
    and the three rows of J = [I, -2[p]x] of J^T J): 2 (N - 1) 2^-53 sum|term| with N the number of non-zero terms of the entry -> f64[6,6]"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    J = np.zeros((p.shape[0], 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, 0, 4], J[:, 0, 5] = 2 * p[:, 2], -2 * p[:, 1]
    J[:, 1, 3], J[:, 1, 5] = -2 * p[:, 2], 2 * p[:, 0]
    J[:, 2, 3], J[:, 2, 4] = 2 * p[:, 1], -2 * p[:, 0]
    terms = np.einsum('nij,nik->nijk', J, J).reshape(-1, 6, 6)
    N = np.count_nonzero(terms, axis=0)
    return 2.0 * np.maximum(N - 1, 0) * U * np.abs(terms).sum(0)
