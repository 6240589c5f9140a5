"""csrc/preprocess.hip against the float64 references of tests/preprocess_ref.py at its seams: (a) buf_knn_normals through the C ABI on
hand-made candidate lists (every arm of the eigen solver, scale and offset, the fp64 re-rank, flags and indirection), (b)
preprocess.estimate_normals against a brute-force k-NN, (c) voxel_down_sample / _batch bit for bit.  Every normal is compared with
normal_ref within angle_bound (constants measured on the CPU, test_preprocess_ref_cpu.py); no row is excused."""
import ctypes as C

import numpy as np
import pytest

import preprocess_ref as ref

pytestmark = pytest.mark.gpu

SENT = 7.0                                  # pre-fill of the normals: a row the kernel must not write keeps it
DEF_SENT = 0xAA                             # pre-fill of the deficient flags
BUF_EINVAL, BUF_EWORKSPACE = -1, -3
CAM = (0.1, -0.2, 0.3)


# ------------------------------------------------------------------------------------------------------------------------------ helpers
def _knn_normals(dev, pts, cand, knn, ns=None, qidx=None, camera=None, orient=0, ncand=None, nq=None):
    """buf_knn_normals through the C ABI -> (rc, normals f32[len(pts),3] pre-filled with SENT, deficient u8[rows] pre-filled)"""
    import torch
    from buffer_amd import _lib
    L = _lib.lib()
    pts = np.ascontiguousarray(pts, np.float32)
    cand = np.ascontiguousarray(cand, np.int32)
    rows = cand.shape[0] if nq is None else nq
    assert qidx is not None or rows <= pts.shape[0]                 # qidx null: row = point (the kernel reads and writes point `row`)
    assert qidx is None or (len(qidx) >= rows and (rows == 0 or (0 <= min(qidx) and max(qidx) < pts.shape[0])))
    p = torch.from_numpy(pts).to(dev)
    c = torch.from_numpy(cand).to(dev) if cand.size else torch.zeros((1,), dtype=torch.int32, device=dev)
    q = None if qidx is None else torch.from_numpy(np.ascontiguousarray(qidx, np.int32)).to(dev)
    normals = torch.full((pts.shape[0], 3), SENT, dtype=torch.float32, device=dev)
    deficient = torch.full((max(cand.shape[0], 1),), DEF_SENT, dtype=torch.uint8, device=dev)
    cam = None if camera is None else (C.c_double * 3)(*[float(v) for v in camera])
    rc = L.buf_knn_normals(p.data_ptr(), pts.shape[0] if ns is None else ns, None if q is None else q.data_ptr(), rows, c.data_ptr(),
                           cand.shape[1] if ncand is None else ncand, knn, cam, orient, normals.data_ptr(), deficient.data_ptr(),
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, normals.cpu().numpy(), deficient.cpu().numpy()


def _pad(rng, valid, ncand, ns):
    """the valid indices in random order with empty slots (ns, ns + 5, -1) between them -> int32[ncand]"""
    row = np.empty(ncand, np.int32)
    slots = rng.permutation(ncand)[:len(valid)]
    row[:] = rng.choice([ns, ns + 5, -1], ncand)
    row[slots] = rng.permutation(np.asarray(valid))
    return row


def _check_rows(group, got, pts, qpts, sets, refs=None, orient=0, camera=CAM):
    """every row qpts[r] of `got` against normal_ref(pts, sets[r]): unit, within angle_bound up to sign, and (orient) with the sign that
    looks at the camera unless n . (cam - q) is itself below the bound.  refs: (n0, lam, mean, bound) per row when already known.
    -> the worst angle / bound (printed for profiles/preprocess_edges.md)"""
    worst = 0.0
    p64 = np.asarray(pts, np.float32).astype(np.float64)
    for r, qi in enumerate(qpts):
        g = got[qi].astype(np.float64)
        assert np.all(np.isfinite(g)) and abs(np.linalg.norm(g) - 1.0) < 1e-6, (group, r, g)
        view = np.asarray(camera, np.float64) - p64[qi]
        if len(sets[r]) < 3:                                        # open3d: covariance = identity -> (0,0,1), then orientation
            want = np.array([0.0, 0.0, -1.0 if orient and view[2] < 0 else 1.0])
            assert np.array_equal(g, want), (group, r, g)
            continue
        if refs is None:
            n0, l0, l1, l2, mean = ref.normal_ref(pts, sets[r])
            bound = ref.angle_bound((l0, l1, l2), mean)
        else:
            n0, bound = refs[0][r], refs[3][r]
        assert bound <= ref.BOUND_CAP, (group, r, bound)            # a condition on the input (checked on the CPU for the random ones)
        a = ref.angle(g, n0)
        assert a <= bound, (group, r, a, bound)
        worst = max(worst, a / bound)
        s = float(n0 @ view)
        if orient and abs(s) > bound * np.linalg.norm(view):
            assert float(g @ view) >= 0.0 and float(g @ n0) * s > 0.0, (group, r, g, n0, s)
    print(f"EDGE_STAT {group}: worst angle/bound {worst:.3g} over {len(qpts)} rows")
    return worst


def _patch_run(dev, name, orient, seed=0, ncand=40):
    """all points of a patch set as queries, candidates = the own patch in random order with empty slots between -> got, reference"""
    pts, sets, n0, lam, mean, bound = ref.patch_reference(name)
    rng = np.random.default_rng(seed)
    ns = pts.shape[0]
    cand = np.stack([_pad(rng, s, ncand, ns) for s in sets])
    scale, shift = ref.PATCH_SETS[name][4], np.asarray(ref.PATCH_SETS[name][5])
    cam = np.asarray(CAM) * scale + shift
    rc, got, deficient = _knn_normals(dev, pts, cand, 30, camera=cam, orient=orient)
    assert rc == 0 and not deficient.any()
    return pts, sets, (n0, lam, mean, bound), got, cam


# ------------------------------------------------------------------------------------------------- (a) solver arms, scale and offset
@pytest.mark.parametrize("name,sign", [("plane", -1), ("needle", 1), ("edge", 1), ("plane_1e-4", -1), ("plane_1e+3", -1), ("plane_shift", -1),
                                       ("needle_1e-4", 1), ("needle_1e+3", 1), ("needle_shift", 1)])
@pytest.mark.parametrize("orient", [0, 1])
def test_knn_normals_solver_arms(dev, name, sign, orient):
    """planar patches (det < 0: eigenvector0 of the smallest eigenvalue), needles and edge-like sets (det >= 0: eigenvector0 of the LARGEST,
    o3d_eigenvector1, cross product), at 1e-4, 1e+3 and translated by (900, -700, 300) (the cumulant cancellation)"""
    pts, sets, refs, got, cam = _patch_run(dev, name, orient)
    assert all(ref.det_sign(l) == sign for l in refs[1]), "the case does not land in its arm"
    _check_rows(f"{name} orient={orient} det{'<0' if sign < 0 else '>=0'}", got, pts, np.arange(pts.shape[0]), sets, refs, orient, cam)


def _lattice_plane(rng, k, z, ylen):
    xy = rng.permutation(64 * 64)[:k]
    return np.stack([(xy % 64) / 64.0 - 0.5, (xy // 64) * (ylen / 64.0), np.full(k, z)], 1).astype(np.float32)


def test_knn_normals_exactly_coplanar(dev):
    """z = 0.5 (a power of two: the cumulants xz, yz, zz cancel exactly), x and y on a lattice: lambda0 = 0, the normal is +-e_z to the fp32
    bound; a square patch (det < 0) and a 1 x 4 strip (det >= 0: the normal is the cross product of the two in-plane eigenvectors)"""
    rng = np.random.default_rng(3)
    pts = np.concatenate([_lattice_plane(rng, 30, 0.5, 1.0), _lattice_plane(rng, 30, 0.5, 4.0) + np.float32([0.25, 1.0, 0.0])])
    sets = [np.arange(30)] * 30 + [np.arange(30, 60)] * 30
    signs = [ref.det_sign(ref.normal_ref(pts, s)[1:4]) for s in (sets[0], sets[30])]
    assert signs == [-1.0, 1.0]
    cand = np.stack([_pad(rng, s, 40, 60) for s in sets])
    for orient in (0, 1):
        rc, got, deficient = _knn_normals(dev, pts, cand, 30, camera=(0.0, 0.0, -3.0), orient=orient)
        assert rc == 0 and not deficient.any()
        _check_rows(f"coplanar orient={orient}", got, pts, np.arange(60), sets, None, orient, (0.0, 0.0, -3.0))
        assert max(ref.angle(g, [0, 0, 1]) for g in got) <= ref.F32_TERM
        assert not orient or np.all(got[:, 2] < 0)


def _axis_lattice(a, b, c, corners=True):
    p = [[a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c], [0, 0, -c]]
    if corners:
        p += [[sx * a, sy * b, sz * c] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return np.array(p, np.float32)


@pytest.mark.parametrize("abc,want", [((1, 2, 3), (1, 0, 0)), ((2, 1, 3), (0, 1, 0)), ((3, 2, 1), (0, 0, 1)),
                                      ((1, 1, 2), (0, 0, 1)), ((1, 2, 1), (0, 0, 1)), ((2, 1, 1), (0, 0, 1)), ((1, 1, 1), (0, 0, 1))])
def test_knn_normals_diagonal_arm(dev, abc, want):
    """sign-symmetric axis lattices centred at the origin: mean and off-diagonal cumulants are exactly 0 in any order of summation
    (norm == 0): the axis of the strictly smallest diagonal entry, e_z on every tie (open3d's rule, restated: for x = y < z that is the axis
    of the LARGEST eigenvalue) and for the isotropic octahedron"""
    pts = _axis_lattice(*abc, corners=abc != (1, 1, 1))
    n = pts.shape[0]
    rng = np.random.default_rng(5)
    cand = np.stack([_pad(rng, np.arange(n), 30, n) for _ in range(n)])
    rc, got, deficient = _knn_normals(dev, pts, cand, n)
    assert rc == 0 and not deficient.any()
    assert np.array_equal(got, np.tile(np.float32(want), (n, 1))), got
    n0, l0, l1, l2, mean = ref.normal_ref(pts, np.arange(n))
    assert np.all(mean == 0)
    if len(set(abc)) == 3:                                          # a strict smallest axis: the reference decides too
        _check_rows(f"diagonal {abc}", got, pts, np.arange(n), [np.arange(n)] * n)
    else:
        assert min(l1 - l0, l2 - l1) < 1e-15                          # a tie: an eigenvalue pair coincides


def test_knn_normals_zero_matrix_and_short_sets(dev):
    """all candidates one identical point (coordinates with few bits: every cumulant cancels exactly) -> zero matrix -> (0,0,1), then
    orientation; knn = 1 and 2 (fewer than 3 points: covariance = identity) -> (0,0,1)"""
    pts = np.concatenate([np.tile(np.float32([0.75, -1.5, 2.25]), (30, 1)), ref.patches('plane')[:30]])
    rng = np.random.default_rng(6)
    cand = np.stack([_pad(rng, np.arange(30), 40, 60) for _ in range(30)])
    rc, got, deficient = _knn_normals(dev, pts, cand, 30)
    assert rc == 0 and not deficient.any() and np.array_equal(got[:30], np.tile(np.float32([0, 0, 1]), (30, 1)))
    rc, got, _ = _knn_normals(dev, pts, cand, 30, camera=(0.0, 0.0, 0.0), orient=1)           # the camera is below the point
    assert rc == 0 and np.array_equal(got[:30], np.tile(np.float32([0, 0, -1]), (30, 1)))
    rc, got, _ = _knn_normals(dev, pts, cand, 30, camera=(0.0, 0.0, 9.0), orient=1)
    assert rc == 0 and np.array_equal(got[:30], np.tile(np.float32([0, 0, 1]), (30, 1)))
    assert np.all(got[30:] == SENT)
    cand = np.stack([_pad(rng, np.arange(30, 60), 40, 60) for _ in range(60)])
    for knn in (1, 2):
        rc, got, deficient = _knn_normals(dev, pts, cand, knn, camera=(0.0, 0.0, -5.0), orient=1)
        assert rc == 0 and not deficient.any() and np.array_equal(got, np.tile(np.float32([0, 0, -1]), (60, 1)))


def test_knn_normals_exactly_collinear(dev):
    """30 points t (1,2,2) + offset, exact in fp32: lambda0 = lambda1 = 0, ANY unit vector across the line is a valid answer and the
    reference cannot say which.  Asserted: finite, unit to 1e-6, orthogonal to the line to 1e-6 -- nothing else is determined."""
    t = np.arange(-15, 15, dtype=np.float64)[:, None]
    rng = np.random.default_rng(7)
    for off in ((0.0, 0.0, 0.0), (0.5, 0.25, -1.0)):
        pts = (t * [1.0, 2.0, 2.0] + off).astype(np.float32)
        cand = np.stack([_pad(rng, np.arange(30), 40, 30) for _ in range(30)])
        rc, got, deficient = _knn_normals(dev, pts, cand, 30)
        assert rc == 0 and not deficient.any()
        g = got.astype(np.float64)
        assert np.all(np.isfinite(g)) and np.all(np.abs(np.linalg.norm(g, axis=1) - 1.0) < 1e-6)
        assert np.all(np.abs(g @ (np.array([1.0, 2.0, 2.0]) / 3.0)) < 1e-6), np.abs(g @ (np.array([1.0, 2.0, 2.0]) / 3.0)).max()


# ---------------------------------------------------------------------------------------------------------------------- (a) the re-rank
def _saddle():
    """a 7 x 7 lattice on the saddle z = x y / 8, points in shuffled order: d2 from the centre ties exactly (in fp32 and fp64) between
    (+-i, +-j) and (+-j, +-i); the shells hold 1, 4, 4, 4, 8, 4, 4, 8, ... points, so a cut at 30 falls inside an eight-fold tie"""
    rng = np.random.default_rng(8)
    ij = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(-3, 4), indexing='ij'), -1).reshape(-1, 2)[rng.permutation(49)]
    return np.concatenate([ij, ij[:, :1] * ij[:, 1:] / 8.0], 1).astype(np.float32)


def test_knn_normals_rerank_ties_and_permutations(dev):
    """the knn nearest are chosen by (fp64 d2, index) among the candidates: with exact ties across the cut the lower index is taken
    (a wrong pick moves the normal of the saddle by ~1e-2 rad), the order of the candidate columns changes nothing -- on this lattice
    every cumulant is a sum of multiples of 1/64 and exact, so not a bit -- and empty slots are skipped"""
    pts = _saddle()
    rng = np.random.default_rng(9)
    cands = [ref.rerank(pts, q, np.arange(49), 48) for q in range(49)]
    sets = [ref.rerank(pts, q, cands[q], 30) for q in range(49)]
    p64 = pts.astype(np.float64)
    d2 = [np.sort(((p64[c] - p64[q]) ** 2).sum(1)) for q, c in enumerate(cands)]
    assert sum(d[29] == d[30] for d in d2) >= 10                       # rows with an exact tie across the cut, the centre among them
    centre = int(np.flatnonzero((pts[:, 0] == 0) & (pts[:, 1] == 0))[0])
    assert d2[centre][29] == d2[centre][30] == d2[centre][36]
    runs = []
    for perm in range(3):
        cand = np.stack([c if perm == 0 else rng.permutation(c) for c in cands])            # run 0: nearest first, as buf_grid_query does
        rc, got, deficient = _knn_normals(dev, pts, cand, 30, camera=(0.0, 0.0, 5.0), orient=1)
        assert rc == 0 and not deficient.any()
        runs.append(got)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)) and np.array_equal(runs[0].view(np.uint32), runs[2].view(np.uint32))
    _check_rows("saddle re-rank", runs[0], pts, np.arange(49), sets, None, 1, (0.0, 0.0, 5.0))
    # the same with empty slots (ns, ns + 5, -1) between the valid ones, 40 of them valid
    cands40 = [c[:40] for c in cands]
    cand = np.stack([_pad(rng, c, 48, 49) for c in cands40])
    rc, got, deficient = _knn_normals(dev, pts, cand, 30, camera=(0.0, 0.0, 5.0), orient=1)
    assert rc == 0 and not deficient.any() and np.array_equal(got.view(np.uint32), runs[0].view(np.uint32))


@pytest.mark.parametrize("ncand,knn", [(1, 1), (30, 30), (30, 23), (40, 40), (40, 33), (48, 48), (48, 41), (48, 30)])
def test_knn_normals_ncand_and_knn(dev, ncand, knn):
    """full rows of ncand candidates (the ncand nearest, shuffled), knn == ncand and knn < ncand"""
    pts = ref.patches('plane_48')
    n = pts.shape[0]
    rng = np.random.default_rng(10)
    cand = np.stack([rng.permutation(ref.rerank(pts, q, np.arange(48 * (q // 48), 48 * (q // 48 + 1)), ncand)) for q in range(n)])
    rc, got, deficient = _knn_normals(dev, pts, cand, knn, camera=CAM, orient=1)
    assert rc == 0 and not deficient.any()
    if knn == 1:
        sets, refs = [np.array([q]) for q in range(n)], None
    else:
        _, sets, *refs = ref.patch_reference('plane_48', knn)
    _check_rows(f"ncand={ncand} knn={knn}", got, pts, np.arange(n), sets, refs, 1, CAM)


# ------------------------------------------------------------------------------------------------------- (a) flags and indirection
def test_knn_normals_deficient_rows_keep_their_output(dev):
    """rows with fewer than min(knn, ns) valid candidates are flagged and NOT written; ns < knn makes need = ns"""
    pts, sets, *refs = ref.patch_reference('plane')
    n = pts.shape[0]
    rng = np.random.default_rng(11)
    short = np.arange(n) % 3 == 1
    cand = np.stack([_pad(rng, s[:29 - (q % 5)] if short[q] else s, 40, n) for q, s in enumerate(sets)])
    rc, got, deficient = _knn_normals(dev, pts, cand, 30)
    assert rc == 0 and np.array_equal(deficient, short.astype(np.uint8))
    assert np.all(got[short] == SENT)
    keep = np.flatnonzero(~short)
    _check_rows("deficient: the other rows", got, pts, keep, [sets[q] for q in keep], [a[keep] for a in refs])
    # need = min(knn, ns): a support of ns = 20 < knn = 30 points (point 0 of 'plane_48' and its 19 nearest): 20 valid slots -> the normal
    # of all 20; 19 valid -> flagged; only slots >= ns -> flagged
    p48, sets20, *refs20 = ref.patch_reference('plane_48', 20)
    sub = p48[sets20[0]]
    cand = np.stack([_pad(rng, np.arange(20), 40, 20), _pad(rng, np.arange(19), 40, 20), np.arange(20, 60)])
    rc, got, deficient = _knn_normals(dev, sub, cand, 30)
    assert rc == 0 and deficient.tolist() == [0, 1, 1] and np.all(got[1:] == SENT)
    assert abs(np.linalg.norm(got[0].astype(np.float64)) - 1.0) < 1e-6 and ref.angle(got[0], refs20[0][0]) <= refs20[3][0]


def test_knn_normals_qidx_and_nq(dev):
    """qidx maps row -> point (only those points are written); qidx null: row = point; nq = 1, 63, 64, 65, 129: one lane per row, 64 rows
    per workgroup, the last workgroup partly filled; nq = 0 writes nothing"""
    pts, sets, *refs = ref.patch_reference('plane_nq')
    n = pts.shape[0]
    rng = np.random.default_rng(12)
    for nq in (1, 63, 64, 65, 129):
        q = np.sort(rng.permutation(n)[:nq]) if nq > 1 else np.array([n - 1])
        for qidx in (q, None):
            qp = q if qidx is not None else np.arange(nq)
            cand = np.stack([_pad(rng, sets[i], 40, n) for i in qp])
            rc, got, deficient = _knn_normals(dev, pts, cand, 30, qidx=qidx, camera=CAM, orient=1)
            assert rc == 0 and not deficient.any() and deficient.shape[0] == nq
            _check_rows(f"nq={nq} qidx={'given' if qidx is not None else 'null'}", got, pts, qp, [sets[i] for i in qp],
                        [a[qp] for a in refs], 1, CAM)
            rest = np.setdiff1d(np.arange(n), qp)
            assert np.all(got[rest] == SENT)
    cand = np.stack([_pad(rng, sets[i], 40, n) for i in range(4)])
    rc, got, deficient = _knn_normals(dev, pts, cand, 30, nq=0)
    assert rc == 0 and np.all(got == SENT) and np.all(deficient == DEF_SENT)


@pytest.mark.parametrize("kw", [dict(orient=1, camera=None), dict(ncand=49), dict(ncand=0), dict(knn=41), dict(knn=0), dict(ns=7)])
def test_knn_normals_rejects_bad_arguments(dev, kw):
    """BUF_EINVAL before anything is launched: the outputs keep their pre-fill.  ns = 7 with 8 rows and no qidx: row = point, so row 7
    would be read and written past the support"""
    pts, sets, *_ = ref.patch_reference('plane')
    rng = np.random.default_rng(13)
    cand = np.stack([_pad(rng, sets[i], 40, pts.shape[0]) for i in range(8)])
    if kw.get('ncand') == 49:
        cand = np.concatenate([cand, cand[:, :9]], 1)
    kw = dict(kw)
    knn = kw.pop('knn', 30)
    rc, got, deficient = _knn_normals(dev, pts, cand, knn, **kw)
    assert rc == BUF_EINVAL
    assert np.all(got == SENT) and np.all(deficient == DEF_SENT)


# ------------------------------------------------------------------------------------------------------------ (b) estimate_normals
def _estimate(dev, pts, **kw):
    import torch
    from buffer_amd import preprocess
    return preprocess.estimate_normals(torch.from_numpy(pts).to(dev), **kw).cpu().numpy()


def _check_cloud(group, got, kind, n, knn, orient=1):
    pts, sets, *refs = ref.cloud_reference(kind, n, knn)
    if kind == 'dup' and n == 3:
        # a point, its copy and one more are collinear: the normal is undetermined (see test_knn_normals_exactly_collinear)
        line = pts[2].astype(np.float64) - pts[0].astype(np.float64)
        g = got.astype(np.float64)
        assert np.all(np.isfinite(g)) and np.all(np.abs(np.linalg.norm(g, axis=1) - 1.0) < 1e-6)
        assert np.all(np.abs(g @ (line / np.linalg.norm(line))) < 1e-6)
        return
    _check_rows(group, got, pts, np.arange(n), sets, refs, orient, CAM)


@pytest.mark.parametrize("n", ref.CLOUD_SIZES)
@pytest.mark.parametrize("kind", ref.CLOUD_KINDS)
def test_estimate_normals_vs_brute_force(dev, kind, n):
    """the pilot radius, the growth rounds and the candidate lists of the cell grid end with every point's exact 30 nearest (by fp64 d2,
    then index): sizes around knn and ncand; a sparse cluster 40 m away (many growth rounds); duplicates and lattice ties"""
    got = _estimate(dev, ref.cloud(kind, n), knn=30, camera=CAM)
    _check_cloud(f"estimate_normals {kind} n={n}", got, kind, n, 30)


@pytest.mark.parametrize("kw", [dict(radius=1e-4), dict(radius=10.0), dict(ncand=48), dict(grow=2.0), dict(knn=3), dict(knn=10), dict(knn=45),
                                dict(orient=False)])
def test_estimate_normals_parameters(dev, kw):
    """radius = 1e-4: dozens of growths; radius = 10: every ball holds the whole cloud (full rows, the 40 nearest); knn = 45 > ncand = 40:
    ncand = max(ncand, knn)"""
    knn = kw.get('knn', 30)
    got = _estimate(dev, ref.cloud('mix', 3000), camera=CAM, **kw)
    _check_cloud(f"estimate_normals mix n=3000 {kw}", got, 'mix', 3000, knn, 1 if kw.get('orient', True) else 0)


@pytest.mark.parametrize("n,knn", [(41, 45), (40, 10)])
def test_estimate_normals_small_clouds_other_knn(dev, n, knn):
    got = _estimate(dev, ref.cloud('mix', n), knn=knn, camera=CAM)
    _check_cloud(f"estimate_normals mix n={n} knn={knn}", got, 'mix', n, knn)


@pytest.mark.parametrize("lengths", [[3000, 0, 500, 31], [3000, 12, 500]])
def test_estimate_normals_stacked_equals_cloud_by_cloud(dev, lengths):
    """[3000, 0, 500, 31]: the stacked path with an empty cloud; [3000, 12, 500]: a cloud of <= knn points sends all of them one by one.
    Bit-equal to separate calls, the first cloud against the reference too; two runs give the same bits"""
    clouds = [ref.cloud('mix', 3000)] + [ref.cloud('two_density' if m == 500 else 'lattice', m, seed=7) for m in lengths[1:]]
    stacked = np.concatenate(clouds)
    got = _estimate(dev, stacked, camera=CAM, lengths=lengths)
    again = _estimate(dev, stacked, camera=CAM, lengths=lengths)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    lo = 0
    for c in clouds:
        if c.shape[0]:
            one = _estimate(dev, c, camera=CAM)
            assert np.array_equal(got[lo:lo + c.shape[0]].view(np.uint32), one.view(np.uint32)), c.shape
        lo += c.shape[0]
    _check_cloud(f"estimate_normals stacked {lengths}: first cloud", got[:3000], 'mix', 3000, 30)


def test_estimate_normals_lengths_must_sum(dev):
    from buffer_amd._lib import BufferHipError
    with pytest.raises(BufferHipError):
        _estimate(dev, ref.cloud('mix', 41), lengths=[30, 12])


# ------------------------------------------------------------------------------------------------------------ (c) voxel_down_sample
def _vds(dev, pts, voxel, normals=None, max_cells=0):
    import torch
    from buffer_amd import preprocess
    out = preprocess.voxel_down_sample(torch.from_numpy(pts).to(dev), voxel, None if normals is None else torch.from_numpy(normals).to(dev),
                                       max_cells=max_cells)
    if normals is None:
        assert out.dtype == torch.float64
        return out.cpu().numpy()
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _seam_cloud(n, dtype, seed=20):
    """a cloud whose bounding box is set by points AT the seams of the partial boxes (256 threads, 64 blocks: indices 0, 255, 256, 16383,
    16384, n - 1): a partial that misses its last or first point moves the origin and with it every voxel"""
    rng = np.random.default_rng(seed + n)
    p = rng.normal(0, 0.4, (n, 3))
    for k, i in enumerate(sorted({0, 255, 256, 16383, 16384, n - 1} & set(range(n)))):
        p[i, k % 3] = (3.0 + 0.37 * k) * (1 if (k // 3) % 2 == 0 else -1)
    p = p.astype(dtype)
    return p + rng.normal(0, 1e-9, p.shape) if dtype == np.float64 else p


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [255, 256, 257, 16383, 16384, 16385])
def test_voxel_down_sample_sizes_at_the_box_seams(dev, n, dtype):
    pts = _seam_cloud(n, dtype)
    nrm = np.random.default_rng(21).normal(size=pts.shape).astype(dtype)
    got, got_n = _vds(dev, pts, 0.11, nrm)
    want, want_n = ref.voxel_means(pts, 0.11, nrm)
    assert 0.2 * n < want.shape[0] < n
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_n, want_n)


def _voxel_case(case):
    rng = np.random.default_rng(22)
    if case == "negative":
        return (rng.random((3000, 3)) * 2.0 - 52.0).astype(np.float32), 0.07
    if case == "straddle":
        return (rng.random((3000, 3)) * 2.0 - 1.0).astype(np.float32), 0.07
    if case == "faces":
        # points EXACTLY on voxel faces: o + k voxel in fp64 with the reference's own o (k >= 1 leaves the minimum, so o, alone)
        base = rng.random((1000, 3)) * 2.0 - 1.0
        o = ref.voxel_origin(base, 0.125)
        on = o + rng.integers(1, 16, (1000, 3)) * 0.125
        mixed = np.where(rng.random((500, 3)) < 0.5, o + rng.integers(1, 16, (500, 3)) * 0.125, rng.random((500, 3)) * 2.0 - 1.0)
        pts = np.concatenate([base, on, mixed])
        assert np.array_equal(ref.voxel_origin(pts, 0.125), o)
        return pts, 0.125
    if case == "faces_third":
        base = rng.random((1000, 3)) * 2.0 - 1.0
        o = ref.voxel_origin(base, 0.1)
        pts = np.concatenate([base, o + rng.integers(1, 20, (1500, 3)) * 0.1])             # 0.1 is no fp64 number: k * 0.1 rounds
        assert np.array_equal(ref.voxel_origin(pts, 0.1), o)
        return pts, 0.1
    if case == "crowd":
        # 5000 points in one voxel (the serial sum of k_o3d_emit, input order) and 1 in another
        p = np.concatenate([0.5 + rng.random((5000, 3)) * 0.01, [[3.0, 3.0, 3.0]]])
        return p[rng.permutation(5001)].astype(np.float32), 0.1
    if case == "one_row":
        return (rng.random((777, 3)) * 2.0 - 1.0).astype(np.float32), 100.0
    if case == "all_rows":
        return rng.random((1000, 3)).astype(np.float32), 1e-6
    if case == "far_f64":
        return 1e6 + rng.random((2000, 3)) * 1e-5, 5e-7                                       # 1e-7 structure on 1e6: fp64 input only
    if case == "outlier":
        return np.concatenate([rng.random((3000, 3)) * 2.0, [[1e4, 1e4, 1e4]]]).astype(np.float32), 0.05
    raise ValueError(case)


@pytest.mark.parametrize("case", ["negative", "straddle", "faces", "faces_third", "crowd", "one_row", "all_rows", "far_f64", "outlier"])
def test_voxel_down_sample_edges(dev, case):
    pts, voxel = _voxel_case(case)
    nrm = np.random.default_rng(23).normal(size=pts.shape).astype(pts.dtype)
    want, want_n = ref.voxel_means(pts, voxel, nrm)
    rows = {"crowd": 2, "one_row": 1, "all_rows": 1000}.get(case)
    assert rows is None or want.shape[0] == rows
    for max_cells in (0, 64) if case in ("outlier", "crowd", "all_rows") else (0,):
        got, got_n = _vds(dev, pts, voxel, nrm, max_cells)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_n, want_n)
    # chained second level on the fp64 means
    np.testing.assert_array_equal(_vds(dev, want, voxel * 1.75), ref.voxel_means(want, voxel * 1.75))


def test_voxel_down_sample_does_not_depend_on_max_cells(dev):
    """the bucket table of the counting sort only buckets: 2 cells put every key in ONE bucket, 3 in two, 64 in a few; the rows are those of
    the default table (heads by (bucket, key), runs in input order)"""
    pts = (np.random.default_rng(24).random((4000, 3)) * 2.0 - 0.7).astype(np.float32)
    nrm = np.random.default_rng(25).normal(size=pts.shape).astype(np.float32)
    want, want_n = ref.voxel_means(pts, 0.1, nrm)
    assert want.shape[0] > 1000
    for max_cells in (2, 3, 64, 1 << 16):
        got, got_n = _vds(dev, pts, 0.1, nrm, max_cells)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_n, want_n)


def test_voxel_down_sample_c_abi_errors(dev):
    """a workspace one byte short: BUF_EWORKSPACE; max_cells = 1: BUF_EINVAL; nothing is written"""
    import torch
    from buffer_amd import _lib
    L = _lib.lib()
    n = 300
    pts = torch.rand((n, 3), device=dev)
    out = torch.full((n, 3), SENT, dtype=torch.float64, device=dev)
    m = C.c_int(-7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = L.buf_voxel_downsample_ws_bytes(n, 1 << 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.buf_voxel_downsample(pts.data_ptr(), None, 0, n, 0.1, out.data_ptr(), None, C.byref(m), 1 << 16, ws.data_ptr(), nbytes - 1, stream)
    assert rc == BUF_EWORKSPACE
    rc = L.buf_voxel_downsample(pts.data_ptr(), None, 0, n, 0.1, out.data_ptr(), None, C.byref(m), 1, ws.data_ptr(), nbytes, stream)
    assert rc == BUF_EINVAL
    torch.cuda.synchronize()
    assert m.value == -7 and bool(torch.all(out == SENT))
    rc = L.buf_voxel_downsample(pts.data_ptr(), None, 0, n, 0.1, out.data_ptr(), None, C.byref(m), 1 << 16, ws.data_ptr(), nbytes, stream)
    torch.cuda.synchronize()
    assert rc == 0 and m.value > 0
    np.testing.assert_array_equal(out[:m.value].cpu().numpy(), ref.voxel_means(pts.cpu().numpy(), 0.1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_down_sample_batch_of_70(dev, dtype):
    """70 clouds of 0, 1, 2, 257 and 1000 points in one call (more clouds than the 64 partial boxes of one): cloud by cloud the rows of
    single calls and of the reference"""
    import torch
    from buffer_amd import preprocess
    rng = np.random.default_rng(26)
    lens = rng.permutation(np.repeat([0, 1, 2, 257, 1000], 14))
    clouds = [((rng.random((m, 3)) * 2.0 - 1.0) * rng.choice([0.5, 1.0, 3.0]) + rng.normal(0, 20.0, 3)).astype(dtype) for m in lens]
    out, out_lens = preprocess.voxel_down_sample_batch(torch.from_numpy(np.concatenate(clouds)).to(dev), lens, 0.13)
    out = out.cpu().numpy()
    lo = 0
    for c, m in zip(clouds, out_lens):
        want = ref.voxel_means(c, 0.13)
        assert int(m) == want.shape[0]
        np.testing.assert_array_equal(out[lo:lo + int(m)], want)
        if c.shape[0]:
            np.testing.assert_array_equal(_vds(dev, c, 0.13), want)
        lo += int(m)
    assert lo == out.shape[0]
