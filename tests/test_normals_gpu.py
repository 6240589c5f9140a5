"""buf_row_normals (include/buffer_hip.h N13, csrc/normals.hip) on the device, through the C entry point with NaN- / 0xAB-prefilled
outputs between guard rows: every case of tests/normals_ref.py (all rows, no sampling) against the centred longdouble reference, the
kernel's seams (n around the wavefront, k_nbr around the LDS tile, max_nn, order, both row-load variants), hand-made rows, the same-bits
rule, and the Python layers above the entry point.  tests/test_normals_cpu.py holds the same cases for the numpy twin."""
import ctypes as C

import numpy as np
import pytest
import torch

import normals_ref as nr
import preprocess_ref as pr

pytestmark = pytest.mark.gpu
ALL_CASES = list(nr.CASES) + list(nr.SMALL_CASES)
NRM_TILE = 32                                                    # csrc/normals.hip: the column tile of the LDS variant


def _entry(dev, pts, nbr, max_nn=0, order=None, camera=None, outputs=('normals', 'cov', 'count')):
    """one buf_row_normals call on prefilled outputs with a guard row on either side -> dict of numpy arrays"""
    from buffer_amd import _lib
    from buffer_amd.ops import _ptr, _stream
    L = _lib.lib()
    P = torch.tensor(np.asarray(pts, np.float32), device=dev)
    R = torch.tensor(np.asarray(nbr, np.int32), device=dev)
    n, k = R.shape
    O = None if order is None else torch.tensor(np.asarray(order, np.int32), device=dev)
    bufs = dict(normals=torch.full((n + 2, 3), float('nan'), dtype=torch.float32, device=dev),
                cov=torch.full((n + 2, 6), float('nan'), dtype=torch.float64, device=dev),
                count=torch.full((n + 2,), -1414812757, dtype=torch.int32, device=dev))                  # 0xABABABAB
    ptr = {k_: (_ptr(b[1:]) if k_ in outputs else None) for k_, b in bufs.items()}
    cam = None if camera is None else (C.c_double * 3)(*[float(c) for c in camera])
    rc = L.buf_row_normals(_ptr(P), n, _ptr(R), k, int(max_nn), _ptr(O), cam, 0 if cam is None else 1, ptr['normals'], ptr['cov'],
                           ptr['count'], _stream())
    assert rc == 0, L.buf_last_error()
    torch.cuda.synchronize()
    out = {}
    for k_, b in bufs.items():
        h = b.cpu().numpy()
        guard = h[[0, -1]]
        assert (np.isnan(guard).all() if k_ != 'count' else (guard == -1414812757).all()), f'{k_}: a guard row was written'
        if k_ not in outputs:
            assert (np.isnan(h).all() if k_ != 'count' else (h == -1414812757).all()), f'{k_}: written although not asked for'
        out[k_] = h[1:-1]
    return out


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=(k != 'count')) for k in a)


@pytest.mark.parametrize('case', ALL_CASES, ids=[nr.case_id(c) for c in ALL_CASES])
def test_every_case_against_the_reference(dev, case):
    """the grid's rows equal the brute-force rows; on them: counts exact, covariance inside the derived bound and the twin's bits,
    angle inside angle_bound on the decided rows, sign where the bound decides it, rows with m < 3 exact"""
    from buffer_amd import ops
    pts, nbr, counts, ref, tw = nr.case_reference(case)
    n, k = nbr.shape
    P = torch.tensor(pts, device=dev)
    grid = ops.CellGrid(P, [n], case[3])
    got_rows, got_counts = grid.query(P, [n], k, q_order=grid.order, counts=True)
    assert np.array_equal(got_rows.cpu().numpy(), nbr) and np.array_equal(got_counts.cpu().numpy(), counts)
    got = _entry(dev, pts, got_rows.cpu().numpy(), 0, grid.order.cpu().numpy(), nr.CAMERA)
    worst = nr.check_outputs(case[3], pts, ref, got['count'], got['cov'], got['normals'], nr.CAMERA)
    same_cov = int((got['cov'] == tw['cov']).all(1).sum())
    same_nrm = int((got['normals'] == tw['normal']).all(1).sum())
    print(f'N13 device {nr.case_id(case)}: worst ratios {worst}; rows with the twin\'s covariance bits {same_cov} / {n}, normal bits {same_nrm} / {n}')
    assert same_cov == n                                        # +, *, / in fp64, a fixed order, no FMA: the twin's bits
    plain = _entry(dev, pts, nbr, 0, None, None)                 # not oriented, no order: the same line
    assert np.array_equal(plain['cov'], got['cov']) and np.array_equal(plain['count'], got['count'])
    assert np.array_equal(np.abs(plain['normals']), np.abs(got['normals']))


@pytest.fixture(scope='module')
def seam_clouds():
    """mix clouds of the seam sizes with their whole rows at radius 0.5 (n <= 100: side 0.3, the rows hold nearly the whole cloud,
    two tiles and more) -> {n: (pts, rows int32[n,longest])}"""
    out = {}
    for n in (1, 63, 64, 65, 129):
        pts = pr.cloud('mix', n)
        out[n] = (pts, nr.rows(pts, 0.5, None)[0])
    return out


def _cut(rows, k, n):
    out = np.full((rows.shape[0], k), n, np.int32)
    w = min(k, rows.shape[1])
    out[:, :w] = rows[:, :w]
    return out


def test_kernel_seams(dev, seam_clouds, monkeypatch):
    """n around the wavefront, k_nbr around the tile and past the longest row, max_nn 0 / below / above k_nbr; per setting the direct and
    the LDS variant, without order, with a random and with a reversed permutation: ten launches, one answer"""
    launches = 0
    for n, (pts, whole) in seam_clouds.items():
        longest = whole.shape[1]
        rng = np.random.default_rng(n)
        orders = (None, rng.permutation(n).astype(np.int32), np.arange(n - 1, -1, -1, dtype=np.int32))
        for k in sorted({1, 3, 16, 17, 30, NRM_TILE, NRM_TILE + 1, 2 * NRM_TILE, 2 * NRM_TILE + 1, longest, longest + 1}):
            nbr = _cut(whole, k, n)
            for max_nn in sorted({0, max(k // 2, 1), k + 5}):
                ref = nr.reference(pts, nbr, max_nn)
                first = None
                for variant in ('direct', 'lds'):
                    monkeypatch.setenv('BUF_N13_ROWS', variant)
                    for order in orders:
                        got = _entry(dev, pts, nbr, max_nn, order, nr.CAMERA)
                        launches += 1
                        if first is None:
                            first = got
                            nr.check_outputs(0.5, pts, ref, got['count'], got['cov'], got['normals'], nr.CAMERA, cap=False)
                            tw = nr.twin(pts, nbr, max_nn, nr.CAMERA)
                            assert np.array_equal(got['cov'], tw['cov']) and np.array_equal(got['count'], tw['count'])
                        else:
                            assert _same(got, first), (n, k, max_nn, variant, order is None)
    print(f'N13 seams: {launches} launches')


def test_variants_and_orders_give_the_same_bits_on_long_rows(dev, monkeypatch):
    """the pure-radius case (rows of up to 123 columns: four tiles, the last one partial), both variants, three orders"""
    from buffer_amd import ops
    case = ('mix', nr.BIG, False, 0.12, None)
    pts, nbr, _, ref, _ = nr.case_reference(case)
    P = torch.tensor(pts, device=dev)
    cell = ops.CellGrid(P, [len(pts)], 0.12).order.cpu().numpy()
    assert np.array_equal(np.sort(cell), np.arange(len(pts)))
    first = None
    for variant in ('direct', 'lds'):
        monkeypatch.setenv('BUF_N13_ROWS', variant)
        for order in (None, cell, cell[::-1].copy()):
            for max_nn in (0, 100):
                got = _entry(dev, pts, nbr, max_nn, order, nr.CAMERA)
                if max_nn:
                    assert np.array_equal(got['count'], np.minimum(ref['m'], 100))
                    continue
                if first is None:
                    first = got
                assert _same(got, first), (variant, order is None)
    again = _entry(dev, pts, nbr, 0, cell, nr.CAMERA)            # a rerun
    assert _same(again, first)


def test_each_output_alone(dev):
    pts, nbr, _, _, _ = nr.case_reference(('mix', 41, False, 0.1, 10))
    full = _entry(dev, pts, nbr, 0, None, nr.CAMERA)
    for name in ('normals', 'cov', 'count'):
        assert np.array_equal(_entry(dev, pts, nbr, 0, None, nr.CAMERA, outputs=(name,))[name], full[name])


def _square(z=0.0):
    return np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z], [5, 5, 5]], np.float32)


def test_hand_made_rows(dev):
    """the hand cases of test_normals_cpu.py on the device: the twin's bits"""
    sq = _square(0.25)
    whole = np.tile(np.array([0, 1, 2, 3], np.int32), (5, 1))
    got = _entry(dev, sq, whole)
    assert got['count'].tolist() == [4] * 5 and np.array_equal(np.abs(got['normals']), np.tile(nr.E_Z.astype(np.float32), (5, 1)))
    assert np.array_equal(got['cov'][0], [0.25, 0.0, 0.0, 0.25, 0.0, 0.0])
    assert (_entry(dev, sq, whole, camera=(0, 0, 9))['normals'][:, 2] == 1.0).all()
    assert (_entry(dev, sq, whole, camera=(0, 0, -9))['normals'][:, 2] == -1.0).all()
    pts = _square()
    few = np.array([[5, 5, 5], [1, 5, 5], [2, 0, 5], [0, 1, 2], [9, -1, 7]], np.int32)
    got = _entry(dev, pts, few, camera=(0, 0, -9))
    assert got['count'].tolist() == [0, 1, 2, 3, 0]
    for i in (0, 1, 2, 4):
        assert np.array_equal(got['cov'][i], nr.IDENTITY6) and got['normals'][i].tolist() == [0.0, 0.0, -1.0]
    holed = np.tile(np.array([0, 5, 1, -1, 2, 1 << 30, 3, -(1 << 31)], np.int32), (5, 1))
    a, b = _entry(dev, pts, whole), _entry(dev, pts, holed)
    assert b['count'].tolist() == [4] * 5 and _same(a, b)
    for max_nn, m in ((4, 2), (5, 3), (99, 4)):
        got = _entry(dev, pts, holed, max_nn)
        tw = nr.twin(pts, holed, max_nn)
        assert got['count'].tolist() == [m] * 5 and np.array_equal(got['cov'], tw['cov'])
    # an order that is no permutation: entries outside [0, n) are skipped, their slots write nothing
    got = _entry(dev, pts, whole, order=np.array([4, -1, 0, 7, 2], np.int32))
    assert got['count'].tolist() == [4, -1414812757, 4, -1414812757, 4] and np.isnan(got['normals'][[1, 3]]).all()


def test_a_row_naming_a_non_finite_point_returns_nan(dev):
    """the NaN rule: NaN outputs for that row and nothing else; through the grid a non-finite point takes the m < 3 rule"""
    from buffer_amd import ops
    pts = _square()
    for bad in (np.nan, np.inf):
        pts[4] = [bad, 0, 0]
        nbr = np.tile(np.array([0, 1, 2, 3], np.int32), (5, 1))
        nbr[1] = [0, 1, 2, 4]
        got = _entry(dev, pts, nbr, camera=(0, 0, 9))
        tw = nr.twin(pts, nbr, camera=(0, 0, 9))
        assert got['count'].tolist() == [4] * 5 and np.isnan(got['normals'][[1, 4]]).all() and np.isnan(got['cov'][1, 0])
        assert np.isfinite(got['normals'][[0, 2, 3]]).all() and np.array_equal(got['cov'], tw['cov'], equal_nan=True)
        P = torch.tensor(pts, device=dev)
        rows = ops.CellGrid(P, [5], 2.0).query(P, [5], 8).cpu().numpy()
        assert np.array_equal(rows, nr.rows(pts, 2.0, 8)[0])
        got = _entry(dev, pts, rows, camera=(0, 0, 9))
        assert got['count'].tolist() == [4, 4, 4, 4, 0] and np.isfinite(got['normals']).all() and np.array_equal(got['cov'][4], nr.IDENTITY6)
        assert got['normals'][4].tolist() == [0.0, 0.0, 1.0]


STACK = (('mix', nr.BIG, False, 0.12, 30), ('two_density', nr.BIG, False, 0.12, 30), ('lattice', nr.BIG, False, 0.2, 30))


@pytest.mark.parametrize('max_nn', [30, None])
def test_a_cloud_alone_and_inside_a_stack_of_three(dev, max_nn):
    """estimate_normals_radius: each cloud alone against the same cloud in a stack of three, in both orders, and a rerun: the same bits;
    with and without a caller's grid; estimate_covariances = the covariances of return_cov"""
    from buffer_amd import ops, preprocess
    clouds = [nr.case_reference(c)[0] for c in STACK]
    r = 0.2                                                      # one radius for the stack
    alone = []
    for p in clouds:
        P = torch.tensor(p, device=dev)
        nrm, cov = preprocess.estimate_normals_radius(P, r, max_nn, camera=nr.CAMERA, return_cov=True)
        assert nrm.dtype == torch.float32 and nrm.shape == (len(p), 3) and cov.dtype == torch.float64 and cov.shape == (len(p), 6)
        alone.append((nrm, cov))
    for perm in ((0, 1, 2), (2, 1, 0)):
        S = torch.from_numpy(np.concatenate([clouds[i] for i in perm])).to(dev)
        lens = [len(clouds[i]) for i in perm]
        nrm, cov = preprocess.estimate_normals_radius(S, r, max_nn, camera=nr.CAMERA, lengths=lens, return_cov=True)
        lo = 0
        for i in perm:
            hi = lo + len(clouds[i])
            assert torch.equal(nrm[lo:hi], alone[i][0]) and torch.equal(cov[lo:hi], alone[i][1]), (perm, i)
            lo = hi
        again = preprocess.estimate_normals_radius(S, r, max_nn, camera=nr.CAMERA, lengths=lens)
        assert torch.equal(again, nrm)
        grid = ops.CellGrid(S, lens, 0.5)                        # a caller's grid with a larger radius
        given, gcov = preprocess.estimate_normals_radius(S, r, max_nn, camera=nr.CAMERA, lengths=lens, grid=grid, return_cov=True)
        assert torch.equal(given, nrm) and torch.equal(gcov, cov)
        assert torch.equal(preprocess.estimate_covariances(S, r, max_nn, lengths=lens, grid=grid), cov)
        assert torch.equal(preprocess.estimate_covariances(S, r, max_nn, lengths=lens), cov)
        with pytest.raises(ValueError, match='does not cover'):
            preprocess.estimate_normals_radius(S, 0.6, max_nn, lengths=lens, grid=grid)
    # against the reference: the first cloud at this radius (rows of the brute force, cut at max_nn)
    rows, _ = nr.rows(clouds[0], r, max_nn)
    ref = nr.reference(clouds[0], rows)
    worst = nr.check_outputs(r, clouds[0], ref, None, alone[0][1].cpu().numpy(), alone[0][0].cpu().numpy(), nr.CAMERA)
    print(f'N13 estimate_normals_radius mix r={r} max_nn={max_nn}: rows of {rows.shape[1]} columns, worst ratios {worst}')
    unoriented = preprocess.estimate_normals_radius(torch.tensor(clouds[0], device=dev), r, max_nn, orient=False)
    assert torch.equal(unoriented.abs(), alone[0][0].abs())


def test_ops_row_normals(dev):
    from buffer_amd import ops
    case = ('two_density', nr.BIG, False, 0.5, 64)
    pts, nbr, _, ref, _ = nr.case_reference(case)
    P, R = torch.tensor(pts, device=dev), torch.tensor(nbr, device=dev)
    base = _entry(dev, pts, nbr, 0, None, nr.CAMERA)
    nrm, cov, cnt = ops.row_normals(P, R, camera=nr.CAMERA, return_cov=True, return_counts=True)
    assert np.array_equal(nrm.cpu().numpy(), base['normals']) and np.array_equal(cov.cpu().numpy(), base['cov'])
    assert np.array_equal(cnt.cpu().numpy(), base['count']) and cnt.dtype == torch.int32
    only = ops.row_normals(P, R, camera=nr.CAMERA, order=torch.arange(len(pts) - 1, -1, -1, dtype=torch.int32, device=dev))
    assert isinstance(only, torch.Tensor) and torch.equal(only, nrm)
    n2, c2 = ops.row_normals(P, R, max_nn=10, return_counts=True)
    assert np.array_equal(c2.cpu().numpy(), np.minimum(ref['m'], 10)) and n2.shape == (len(pts), 3)


def test_open3d_standin(dev):
    """the stand-in's three search parameters and covariances"""
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import preprocess
    g = o3d.geometry
    pts = nr.case_reference(('mix', nr.BIG, False, 0.12, 30))[0]
    P = torch.tensor(pts, device=dev)
    pcd = g.PointCloud(pts.astype(np.float64))
    assert pcd.estimate_normals(g.KDTreeSearchParamHybrid(radius=0.12, max_nn=30)) is pcd and pcd.has_normals()
    want, cov = preprocess.estimate_normals_radius(P, 0.12, 30, orient=False, return_cov=True)
    assert np.array_equal(np.asarray(pcd.normals), want.cpu().numpy().astype(np.float64))
    pcd.estimate_normals(g.KDTreeSearchParamRadius(0.12))
    assert np.array_equal(np.asarray(pcd.normals), preprocess.estimate_normals_radius(P, 0.12, None, orient=False).cpu().numpy().astype(np.float64))
    pcd.estimate_normals(g.KDTreeSearchParamKNN(30))
    knn = preprocess.estimate_normals(P, knn=30, orient=False).cpu().numpy().astype(np.float64)
    assert np.array_equal(np.asarray(pcd.normals), knn)
    pcd.estimate_normals()
    assert np.array_equal(np.asarray(pcd.normals), knn)
    assert pcd.estimate_covariances(g.KDTreeSearchParamHybrid(0.12, 30)) is pcd and pcd.has_covariances()
    c = cov.cpu().numpy()
    assert pcd.covariances.shape == (len(pts), 3, 3) and np.array_equal(pcd.covariances, np.swapaxes(pcd.covariances, 1, 2))
    assert np.array_equal(pcd.covariances[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], c)
    pcd.estimate_covariances(g.KDTreeSearchParamRadius(0.12))
    assert np.array_equal(pcd.covariances[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], preprocess.estimate_covariances(P, 0.12, None).cpu().numpy())
    pcd.orient_normals_towards_camera_location(nr.CAMERA)        # orientation stays a separate call
    assert ((np.asarray(pcd.normals) * (np.asarray(nr.CAMERA) - pts.astype(np.float64))).sum(1) >= 0).all()
