"""The numpy twin of buf_row_normals (tests/normals_ref.py: include/buffer_hip.h N13 restated) against the centred longdouble reference
on every case the device suites use, hand cases whose answer is known, and the host side of the feature: every BUF_EINVAL of the entry
point with its full message (dummy pointers: all of them are decided before any device work), the Python argument checks, the ctypes
signature, the stand-in's entries and the drivers' options.  No device."""
import ctypes as C

import numpy as np
import pytest

import normals_ref as nr
import preprocess_ref as pr

ALL_CASES = list(nr.CASES) + list(nr.SMALL_CASES)


@pytest.mark.parametrize('case', ALL_CASES, ids=[nr.case_id(c) for c in ALL_CASES])
def test_twin_against_the_centred_reference(case):
    """every row of every case (no sampling): counts pinned, covariance inside the derived bound, angle inside angle_bound on the decided
    rows, sign as the reference's wherever the bound decides it, rows of fewer than 3 points exact"""
    pts, nbr, counts, ref, tw = nr.case_reference(case)
    few = int((ref['m'] < 3).sum())
    undecided = int(((ref['m'] >= 3) & (ref['bound'] > pr.BOUND_CAP)).sum())
    assert nbr.shape == (case[1], case[4] if case[4] is not None else max(int(counts.max()), 1))
    assert np.array_equal(ref['m'], np.minimum(counts, nbr.shape[1]))            # the rows hold no hole: m = the row's length, cut
    if case in nr.CASES:
        assert (few, undecided, int(counts.max())) == nr.CASES[case]
    else:
        assert few == nr.SMALL_CASES[case] and undecided == 0
    worst = nr.check_outputs(case[3], pts, ref, tw['count'], tw['cov'], tw['normal'], nr.CAMERA)
    print(f'N13 twin {nr.case_id(case)}: {few} rows with m < 3, {undecided} undecided, longest row {int(counts.max())}, worst ratios {worst}')
    assert worst.get('angle', 0.0) <= 0.5 and worst['cov'] <= 0.5               # (the twin sits well inside: 0.26 and 0.11 at most)


def test_query_centred_moments_beat_raw_cumulants_on_the_translated_cloud():
    """the stated deviation: about the query point the covariance of the cloud moved by SHIFT is as exact as at the origin"""
    case = ('mix', nr.BIG, True, 0.12, 30)
    pts, nbr, _, ref, tw = nr.case_reference(case)
    P = pts.astype(np.float64)
    sets = ref['sets']
    raw = np.array([[np.mean(P[s][:, a] * P[s][:, b]) - P[s][:, a].mean() * P[s][:, b].mean() for a, b in nr.PAIRS] for s in sets[::50]])
    err_raw = np.abs(raw - ref['cov'][::50]).max()
    err_twin = np.abs(tw['cov'] - ref['cov']).max()
    assert err_twin <= nr.cov_bound(30, 0.12) and err_raw > 1e4 * err_twin, (err_raw, err_twin)


def _square(z=0.0):
    return np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z], [5, 5, 5]], np.float32)


def test_coplanar_square_gives_exactly_e_z():
    pts = _square(0.25)
    nbr = np.tile(np.array([0, 1, 2, 3], np.int32), (5, 1))
    tw = nr.twin(pts, nbr)
    assert tw['count'].tolist() == [4] * 5
    assert np.array_equal(np.abs(tw['normal']), np.tile(nr.E_Z.astype(np.float32), (5, 1)))
    assert np.array_equal(tw['cov'][0], [0.25, 0.0, 0.0, 0.25, 0.0, 0.0])        # about corner 0: E = (.5, .25, 0, .5, 0, 0), mu = (.5, .5, 0)
    up, down = nr.twin(pts, nbr, camera=(0, 0, 9))['normal'], nr.twin(pts, nbr, camera=(0, 0, -9))['normal']
    assert (up[:, 2] == 1.0).all() and (down[:, 2] == -1.0).all()


def test_rows_of_fewer_than_three_points():
    pts = _square()
    nbr = np.array([[5, 5, 5], [1, 5, 5], [2, 0, 5], [0, 1, 2], [9, -1, 7]], np.int32)
    tw = nr.twin(pts, nbr, camera=(0, 0, -9))
    assert tw['count'].tolist() == [0, 1, 2, 3, 0]
    for i in (0, 1, 2, 4):
        assert np.array_equal(tw['cov'][i], nr.IDENTITY6) and tw['normal'][i].tolist() == [0.0, 0.0, -1.0]       # (0, 0, 1), then oriented
    assert tw['normal'][3, 2] == -1.0 and np.abs(tw['normal'][3, :2]).max() < 1e-7 and not np.array_equal(tw['cov'][3], nr.IDENTITY6)


def test_row_with_a_hole_and_bad_indices_in_the_middle():
    pts = _square()
    whole = np.tile(np.array([0, 1, 2, 3], np.int32), (5, 1))
    holed = np.tile(np.array([0, 5, 1, -1, 2, 1 << 30, 3, -(1 << 31)], np.int32), (5, 1))
    a, b = nr.twin(pts, whole), nr.twin(pts, holed)
    assert b['count'].tolist() == [4] * 5
    assert np.array_equal(a['cov'], b['cov']) and np.array_equal(a['normal'], b['normal'])    # the valid entries, in column order
    cut = nr.twin(pts, holed, max_nn=4)                                                      # columns 0..3: points 0 and 1 only
    assert cut['count'].tolist() == [2] * 5 and np.array_equal(cut['cov'], np.tile(nr.IDENTITY6, (5, 1)))
    assert nr.twin(pts, holed, max_nn=5)['count'].tolist() == [3] * 5 and nr.twin(pts, holed, max_nn=99)['count'].tolist() == [4] * 5


def test_a_hand_made_row_naming_a_non_finite_point_gives_nan():
    pts = _square()
    pts[4] = [np.nan, 0, 0]
    nbr = np.tile(np.array([0, 1, 2, 4], np.int32), (5, 1))
    tw = nr.twin(pts, nbr)
    assert tw['count'].tolist() == [4] * 5 and np.isnan(tw['normal']).all() and np.isnan(tw['cov'][:, 0]).all()
    grid_rows, _ = nr.rows(pts, 2.0, 8)                          # the grid's rows: the NaN point is alone and in no row
    assert (grid_rows[4] == 5).all() and not (grid_rows == 4).any()
    tw = nr.twin(pts, grid_rows)
    assert tw['count'].tolist() == [4, 4, 4, 4, 0] and np.isfinite(tw['normal']).all() and np.array_equal(tw['cov'][4], nr.IDENTITY6)


def test_sums_run_in_column_order():
    pts = np.array([[0, 0, 0], [1e8, 0, 0], [1, 0, 0], [-1e8, 0, 0]], np.float32)
    big = float(np.float32(1e8))
    for row in ([0, 1, 2, 3], [0, 1, 3, 2], [2, 0, 1, 3]):
        s1 = s2 = 0.0
        for j in row:
            d = float(pts[j, 0])
            s1 += d
            s2 += d * d
        got = nr.twin(pts, np.tile(np.array(row, np.int32), (4, 1)))['cov'][0, 0]
        assert got == s2 / 4 - (s1 / 4) * (s1 / 4)
    assert big * big + 1.0 == big * big                         # the order matters for these numbers


# ------------------------------------------------------------------------------------------------------------------------ the entry point
def _bad_calls():
    dummy = (C.c_double * 16)()
    x = C.addressof(dummy)
    order = ('pts', 'n', 'nbr', 'k_nbr', 'max_nn', 'order', 'camera', 'orient', 'normals', 'cov', 'count', 'stream')
    base = dict(pts=x, n=5, nbr=x, k_nbr=4, max_nn=0, order=None, camera=x, orient=1, normals=x, cov=x, count=x, stream=None)
    cases = [
        ('negative n', dict(n=-1), 'buf_row_normals: n=-1'),
        ('k_nbr 0', dict(k_nbr=0), 'buf_row_normals: k_nbr=0'),
        ('negative max_nn', dict(max_nn=-1), 'buf_row_normals: max_nn=-1'),
        ('no output', dict(normals=None, cov=None, count=None), 'buf_row_normals: null outputs normals_out, cov_out and count_out'),
        ('orient without a camera', dict(camera=None), 'buf_row_normals: null camera_host with orient=1'),
        ('null pts', dict(pts=None), 'buf_row_normals: null input pts'),
        ('null nbr', dict(nbr=None), 'buf_row_normals: null input nbr'),
        ('n before k_nbr', dict(n=-2, k_nbr=0), 'buf_row_normals: n=-2'),
        ('k_nbr before the outputs', dict(k_nbr=-3, normals=None, cov=None, count=None), 'buf_row_normals: k_nbr=-3'),
        ('the outputs before the inputs', dict(pts=None, normals=None, cov=None, count=None),
         'buf_row_normals: null outputs normals_out, cov_out and count_out'),
    ]
    return [(label, tuple({**base, **over}[k] for k in order), text) for label, over, text in cases], dummy


_CALLS, _KEEP = _bad_calls()


@pytest.mark.parametrize('label,args,text', _CALLS, ids=[c[0] for c in _CALLS])
def test_einval_and_message(label, args, text):
    from buffer_amd import _lib
    L = _lib.lib()
    assert L.buf_row_normals(*args) == -1 and (L.buf_last_error() or b'').decode() == text


def test_no_points_succeed_and_touch_nothing():
    from buffer_amd import _lib
    L = _lib.lib()
    guard = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    x = C.addressof(guard)
    assert L.buf_row_normals(None, 0, None, 1, 0, None, None, 0, x, x, x, None) == 0
    assert L.buf_row_normals(None, 0, None, 1, 30, None, x, 1, None, None, x, None) == 0
    assert list(guard) == [7.0] * 4


def test_ctypes_signature_header_and_version():
    import os
    from buffer_amd import _lib
    assert 'buf_row_normals' in set(_lib.exported_symbols())
    fn = _lib.lib().buf_row_normals
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    assert _lib.lib().buf_version() == 670
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'buffer_hip.h')).read()
    assert '/* N13 ' in hdr and 'int     buf_row_normals(const float* pts, int n, const int* nbr, int k_nbr, int max_nn' in hdr


def _on_host(mod):
    """step over the device check of the arguments (everything asked for here is decided before the first device call)"""
    real = mod._dev
    mod._dev = lambda t, dtype, what: t.to(dtype).contiguous()
    return real


def test_python_argument_checks():
    import torch
    from buffer_amd import ops, preprocess
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(_lib_error(), match='device memory'):
        ops.row_normals(f32(5, 3), i32(5, 4))
    real, real_p = _on_host(ops), _on_host(preprocess)
    try:
        for args, kw, text in (((f32(5, 4), i32(5, 4)), {}, r'row_normals: points \(5, 4\) is not \[N,3\]'),
                               ((f32(5, 3), i32(4, 4)), {}, r'row_normals: nbr \(4, 4\) is not \[5,k\], k >= 1'),
                               ((f32(5, 3), i32(5, 0)), {}, r'row_normals: nbr \(5, 0\) is not \[5,k\], k >= 1'),
                               ((f32(5, 3), i32(20)), {}, r'row_normals: nbr \(20,\) is not \[5,k\], k >= 1'),
                               ((f32(5, 3), i32(5, 4)), dict(max_nn=-1), r'row_normals: max_nn=-1'),
                               ((f32(5, 3), i32(5, 4)), dict(order=i32(4)), r'row_normals: order \(4,\) is not \[5\]'),
                               ((f32(5, 3), i32(5, 4)), dict(camera=(0, 0)), r'row_normals: camera holds 2 numbers, not 3')):
            with pytest.raises(ValueError, match=text):
                ops.row_normals(*args, **kw)
        for fn in (preprocess.estimate_normals_radius, preprocess.estimate_covariances):
            name = fn.__name__
            for args, kw, text in (((f32(5, 2), 0.1), {}, rf'{name}: points \(5, 2\) is not \[N,3\]'),
                                   ((f32(5, 3), 0.1), dict(lengths=[2, 2]), rf'{name}: lengths sum to 4, points holds 5 rows'),
                                   ((f32(5, 3), 0.0), {}, rf'{name}: radius=0.0 \(finite, > 0\)'),
                                   ((f32(5, 3), float('inf')), {}, rf'{name}: radius=inf'),
                                   ((f32(5, 3), float('nan')), {}, rf'{name}: radius=nan'),
                                   ((f32(5, 3), 0.1), dict(max_nn=0), rf'{name}: max_nn=0 \(None or >= 1\)')):
                with pytest.raises(ValueError, match=text):
                    fn(*args, **kw)

            class Grid:
                radius, ns, s_lengths = 0.05, 5, np.array([5], np.int32)
            with pytest.raises(ValueError, match=rf'{name}: the given grid does not cover'):
                fn(f32(5, 3), 0.1, grid=Grid())                  # a grid at a smaller radius
            Grid.radius, Grid.ns = 0.2, 6
            with pytest.raises(ValueError, match=rf'{name}: the given grid does not cover'):
                fn(f32(5, 3), 0.1, grid=Grid())                  # a grid over other points
        # no points: the empty result, no device
        assert preprocess.estimate_normals_radius(f32(0, 3), 0.1).shape == (0, 3)
        n0, c0 = preprocess.estimate_normals_radius(f32(0, 3), 0.1, max_nn=None, return_cov=True)
        assert n0.shape == (0, 3) and c0.shape == (0, 6) and c0.dtype == torch.float64
        assert preprocess.estimate_covariances(f32(0, 3), 0.1).shape == (0, 6)
    finally:
        ops._dev, preprocess._dev = real, real_p


def _lib_error():
    from buffer_amd import _lib
    return _lib.BufferHipError


def test_existing_estimate_normals_keeps_its_signature():
    import inspect
    from buffer_amd import preprocess
    assert str(inspect.signature(preprocess.estimate_normals)) == \
        '(points, knn=30, camera=(0.0, 0.0, 0.0), orient=True, radius=None, ncand=40, grow=1.35, lengths=None)'
    assert str(inspect.signature(preprocess.estimate_normals_radius)) == \
        '(points, radius, max_nn=30, camera=(0.0, 0.0, 0.0), orient=True, lengths=None, grid=None, return_cov=False)'
    assert str(inspect.signature(preprocess.estimate_covariances)) == \
        '(points, radius, max_nn=30, camera=(0.0, 0.0, 0.0), orient=True, lengths=None, grid=None)'


def test_standin_entries():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    g = o3d.geometry
    pcd = g.PointCloud(np.zeros((4, 3)))
    assert pcd.covariances.shape == (0, 3, 3) and not pcd.has_covariances()
    for call in (lambda: pcd.estimate_covariances(), lambda: pcd.estimate_covariances(g.KDTreeSearchParamKNN(30)),
                 lambda: pcd.estimate_normals(object())):
        with pytest.raises(NotImplementedError, match='KDTreeSearchParamHybrid or KDTreeSearchParamRadius'):
            call()
    pcd.covariances = np.tile(np.eye(3), (4, 1, 1))
    assert pcd.has_covariances() and pcd.covariances.shape == (4, 3, 3)
    assert 'estimate_covariances' in o3d.__doc__ and 'KDTreeSearchParamRadius' in o3d.__doc__


def test_refine_and_registration_options():
    import torch
    from buffer_amd import fpfh, pipeline
    from buffer_amd.config import THREEDMATCH
    assert pipeline.REFINE_NORMALS == ('knn', 'hybrid') and fpfh.NORMALS == ('given', 'hybrid')
    pipe = pipeline.BufferPipeline.__new__(pipeline.BufferPipeline)           # the checks need no state
    pipe.device = torch.device('cpu')
    with pytest.raises(ValueError, match="unknown normals 'radius'"):
        pipe.refine_batch([], [], normals='radius')
    assert pipe.refine_batch([], [], normals='hybrid', normal_radius=0.2, normal_max_nn=20)['poses'].shape == (0, 4, 4)
    with pytest.raises(ValueError, match="unknown normals 'knn'"):
        fpfh.FpfhRegistration(THREEDMATCH, 'cuda:0', normals='knn')


def test_driver_options(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert (a.refine_normals, a.refine_normal_radius, a.fpfh_normals) == ('knn', None, 'given')
        a, _ = mod.parse_args(['--root', 'r', '--refine', 'generalized', '--refine-normals', 'hybrid', '--refine-normal-radius', '0.25'])
        assert (a.refine_normals, a.refine_normal_radius) == ('hybrid', 0.25)
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--fpfh-normals', 'hybrid', '--refine', 'point_to_plane'])
        assert a.fpfh_normals == 'hybrid' and a.refine_normals == 'knn'
        for argv, text in ((['--fpfh-normals', 'hybrid'], '--fpfh-normals hybrid'),
                           (['--refine-normals', 'hybrid'], '--refine-normals hybrid'),
                           (['--descriptor', 'fpfh', '--refine', 'generalized', '--refine-normals', 'hybrid'], '--refine-normals hybrid'),
                           (['--refine', 'generalized', '--refine-normal-radius', '0.2'], '--refine-normal-radius 0.2'),
                           (['--refine', 'generalized', '--refine-normals', 'hybrid', '--refine-normal-radius', '-1'], 'must be finite and > 0')):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(['--root', 'r'] + argv)
            assert e.value.code == 2 and text in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--refine', 'generalized', '--refine-normals', 'pca'])
