"""TEST INFRASTRUCTURE: the references of buf_row_normals (include/buffer_hip.h N13) in plain numpy, and the cases its suites share.

    rows(pts, radius, max_nn, lengths)   the neighbour rows buf_grid_query gives: radius_ref.brute_force (the grid's fp32 rule restated)
                                         cut at max_nn, or at the longest row for max_nn=None; compared exactly
    reference(pts, nbr, max_nn)          per row the expected normal, eigenvalues, mean and angle bound (preprocess_ref.normal_ref:
                                         centred, np.longdouble) and the centred longdouble covariance
    twin(pts, nbr, max_nn, camera)       N13 itself: the sums about the query point in column order, one numpy operation per column
                                         (elementwise fp64, nothing fused), the solver = oracle.cpu.o3d_fast_eigen3x3

Bounds.  Angle: preprocess_ref.angle_bound, whose constants were measured on the CPU for the raw-cumulant form E[x x^T] - m m^T about
the origin; N13 takes the moments about the query point, |mean - q| <= r instead of |mean|, and only errs less.  Covariance, per entry:
cov_bound(m, r) = (m + 4) * 2**-53 * r**2 -- the rounding of at most m additions of terms <= r**2, then the division and the product
(r: a length no neighbour of the row exceeds, the search radius for grid rows).
Undecided rows: angle_bound > preprocess_ref.BOUND_CAP; at most CAP_FRACTION of a case's rows with m >= 3 may be undecided."""
import functools

import numpy as np

import preprocess_ref as pr
import radius_ref

CAP_FRACTION = 0.01
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
IDENTITY6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
E_Z = np.array([0.0, 0.0, 1.0])


def rows(pts, radius, max_nn=None, lengths=None):
    """-> (nbr int32[n,k] padded with n, untruncated counts int32[n]); k = max_nn, or the longest row (>= 1) for max_nn=None"""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    lens = [len(p)] if lengths is None else list(lengths)
    table, counts, mc = radius_ref.brute_force(p, p, lens, lens, radius)
    k = max(mc, 1) if max_nn is None else int(max_nn)
    return radius_ref.expected((table, counts, mc), k, len(p)), counts


def columns(nbr, n, max_nn):
    nbr = np.asarray(nbr).reshape(n, -1)
    kmax = nbr.shape[1] if not max_nn else min(int(max_nn), nbr.shape[1])
    nbr = nbr[:, :kmax].astype(np.int64)
    return nbr, (nbr >= 0) & (nbr < n)


def sets_of(nbr, n, max_nn=0):
    nb, valid = columns(nbr, n, max_nn)
    return [nb[i][valid[i]] for i in range(n)]


def cov_bound(m, r):
    return (np.asarray(m, np.float64) + 4.0) * pr.EPS53 * float(r) ** 2


def reference(pts, nbr, max_nn=0):
    """-> dict(sets, m int64[n], n0 f64[n,3], lam f64[n,3], mean f64[n,3], bound f64[n] (inf where m < 3), cov f64[n,6] (the identity
    where m < 3))"""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    sets = sets_of(nbr, len(p), max_nn)
    n0, lam, mean, bound = pr.rows_ref(p, sets)
    cov = np.tile(IDENTITY6, (len(p), 1))
    for i, s in enumerate(sets):
        if len(s) >= 3:
            x = p[s].astype(np.longdouble)
            c = x - x.sum(0) / len(s)
            full = (c.T @ c) / len(s)
            cov[i] = [float(full[a, b]) for a, b in PAIRS]
    return dict(sets=sets, m=np.array([len(s) for s in sets], np.int64), n0=n0, lam=lam, mean=mean, bound=bound, cov=cov)


def twin(pts, nbr, max_nn=0, camera=None):
    """N13 in numpy -> dict(count int32[n], cov f64[n,6], normal f32[n,3])"""
    from oracle import cpu
    P = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(P)
    nb, valid = columns(nbr, n, max_nn)
    m = valid.sum(1)
    S1, S2 = np.zeros((n, 3)), np.zeros((n, 6))
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(nb.shape[1]):
            v = valid[:, c]
            d = P[nb[v, c]] - P[v]
            S1[v] = S1[v] + d
            for e, (a, b) in enumerate(PAIRS):
                S2[v, e] = S2[v, e] + d[:, a] * d[:, b]
        dm = np.maximum(m, 1).astype(np.float64)[:, None]
        mu, E = S1 / dm, S2 / dm
        cov = np.stack([E[:, e] - mu[:, a] * mu[:, b] for e, (a, b) in enumerate(PAIRS)], 1)
    cov[m < 3] = IDENTITY6
    nrm = np.tile(E_Z, (n, 1))
    for i in np.flatnonzero(m >= 3):
        if np.isfinite(cov[i]).all():
            v = cpu.o3d_fast_eigen3x3(cov[i])
            nrm[i] = v if (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) != 0.0 else E_Z
        else:
            nrm[i] = np.nan
    if camera is not None:
        r = np.asarray(camera, np.float64).reshape(1, 3) - P
        with np.errstate(invalid='ignore'):
            dot = (nrm[:, 0] * r[:, 0] + nrm[:, 1] * r[:, 1]) + nrm[:, 2] * r[:, 2]
        nrm[dot < 0.0] *= -1.0
    return dict(count=m.astype(np.int32), cov=cov, normal=nrm.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the cases of the suites
# (cloud of preprocess_ref.cloud, n, shifted by preprocess_ref.SHIFT, radius, max_nn) -> pinned (rows with m < 3, undecided rows, longest
# row of the radius before the cut at max_nn).  The counts are those of preprocess_ref.cloud's draws as they stand.
BIG = 3000
CASES = {
    ('mix', BIG, False, 0.12, 30): (0, 0, 123),
    ('mix', BIG, False, 0.12, None): (0, 0, 123),
    ('mix', BIG, False, 0.05, 30): (204, 0, 58),
    ('mix', BIG, False, 0.3, 100): (0, 0, 289),
    ('mix', BIG, True, 0.12, 30): (0, 0, 123),
    ('two_density', BIG, False, 0.12, 30): (52, 0, 29),
    ('two_density', BIG, False, 0.5, 64): (8, 0, 261),
    ('dup', BIG, False, 0.12, 30): (0, 2, 132),
    ('lattice', BIG, False, 0.2, 30): (0, 0, 37),
    ('lattice', BIG, False, 0.2, None): (0, 0, 37),
}
# the small clouds -> pinned rows with m < 3 (none of their rows is undecided)
_SMALL_FEW = {(2, 0.1): 2, (2, 0.5): 2, (3, 0.1): 3, (3, 0.5): 0, (40, 0.1): 3, (40, 0.5): 0, (41, 0.1): 0, (41, 0.5): 0}
SMALL_CASES = {('mix', n, False, r, k): _SMALL_FEW[(n, r)] for n in (2, 3, 40, 41) for r in (0.1, 0.5) for k in (10, 30)}
CAMERA = (0.3, -0.2, 4.0)


def case_id(case):
    kind, n, shifted, r, k = case
    return f"{kind}{'_shift' if shifted else ''}-{n}-r{r}-nn{k}"


def case_cloud(case):
    kind, n, shifted = case[:3]
    p = pr.cloud(kind, n)
    if shifted:
        p = (p.astype(np.float64) + np.asarray(pr.SHIFT)).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """-> (pts, nbr, untruncated counts, reference dict, twin dict oriented to CAMERA); shared, never modified"""
    pts = case_cloud(case)
    nbr, counts = rows(pts, case[3], case[4])
    for a in (pts, nbr, counts):
        a.setflags(write=False)
    return pts, nbr, counts, reference(pts, nbr), twin(pts, nbr, 0, CAMERA)


def check_outputs(r, pts, ref, got_count, got_cov, got_normal, camera, cap=True):
    """the assertions every layer shares, for rows of a search at radius r -> dict of the worst ratios.  got_*: numpy arrays (None: not
    checked); camera: what the normals were oriented to (None: left as computed).  cap=False: the seam tests, whose rows are cut down
    to 3 columns and fewer on purpose -- thin triangles whose normal no bound decides; counts and covariances cover those rows."""
    m, bound = ref['m'], ref['bound']
    out = {}
    if got_count is not None:
        assert np.array_equal(got_count, m.astype(np.int32))
    few = m < 3
    decided = ~few & (bound <= pr.BOUND_CAP)
    assert not cap or (~few & ~decided).sum() <= CAP_FRACTION * max(int((~few).sum()), 1)
    if got_cov is not None:
        assert np.array_equal(got_cov[few], np.tile(IDENTITY6, (int(few.sum()), 1)))
        err = np.abs(got_cov - ref['cov']).max(1)
        ratio = err[~few] / cov_bound(m[~few], r)
        out['cov'] = float(ratio.max()) if ratio.size else 0.0
        assert (ratio <= 1.0).all(), out
    if got_normal is not None:
        assert got_normal.dtype == np.float32
        P = np.asarray(pts, np.float32).astype(np.float64)
        view = np.asarray(camera, np.float64).reshape(1, 3) - P if camera is not None else None
        want_few = np.tile(E_Z, (int(few.sum()), 1))
        if view is not None:
            want_few[(view[few] @ E_Z) < 0.0] *= -1.0
        assert np.array_equal(got_normal[few].astype(np.float64), want_few)
        worst, signs = 0.0, 0
        for i in np.flatnonzero(decided):
            g = got_normal[i].astype(np.float64)
            assert abs(np.linalg.norm(g) - 1.0) < 1e-6
            a = pr.angle(g, ref['n0'][i])
            worst = max(worst, a / bound[i])
            assert a <= bound[i], (i, a, bound[i])
            if view is not None:
                s = float(ref['n0'][i] @ view[i])
                if abs(s) > bound[i] * np.linalg.norm(view[i]):
                    signs += 1
                    assert np.sign(float(g @ ref['n0'][i])) == np.sign(s), i
        out['angle'], out['signs'] = worst, signs
    return out
