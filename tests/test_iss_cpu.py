"""The float64 restatement of the ISS contract (tests/iss_ref.py) pinned on shapes whose answer is known by hand, and the host-side
pieces of the detector: the --keypoints option, the ctypes signature, the open3d stand-in's entry.  No device."""
import ctypes as C

import numpy as np
import pytest

import iss_ref


def _box_corner(step=0.05, size=0.5):
    """the three faces of a box that meet in the corner (0, 0, 0), on a lattice, with a little seeded jitter (exact planes have
    l3 = rounding noise)"""
    g = np.arange(0.0, size + 1e-9, step)
    u, v = (a.ravel() for a in np.meshgrid(g, g, indexing='ij'))
    z = np.zeros_like(u)
    pts = np.unique(np.concatenate([np.stack([u, v, z], 1), np.stack([u, z, v], 1), np.stack([z, u, v], 1)]), axis=0)
    return (pts + np.random.default_rng(0).normal(scale=0.002, size=pts.shape)).astype(np.float32)


def test_covariance_and_eigenvalues_by_hand():
    # the six points +-e_a scaled by (3, 2, 1): mean 0, C = diag(9, 4, 1) * 2 / 6
    pts = np.array([[3, 0, 0], [-3, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    rows = np.tile(np.arange(6, dtype=np.int32), (6, 1))
    m, Cv = iss_ref.covariance(pts, rows)
    assert (m == 6).all() and np.array_equal(Cv[0], [3.0, 0, 0, 4.0 / 3.0, 0, 1.0 / 3.0])
    r = iss_ref.iss(pts, rows, rows, min_neighbors=5)
    assert np.allclose(r['eig'], [[3.0, 4.0 / 3.0, 1.0 / 3.0]] * 6, rtol=1e-15)
    assert np.array_equal(r['saliency'], r['eig'][:, 2]) and r['mask'].all()            # all tie: ties keep every point
    assert not iss_ref.iss(pts, rows, rows, min_neighbors=7)['mask'].any()                 # six neighbours are too few
    # l2 / l1 = 4 / 9: gamma_21 = 0.4 rejects, 0.45 accepts; l3 / l2 = 1 / 4
    assert not iss_ref.iss(pts, rows, rows, gamma_21=0.4)['saliency'].any()
    assert iss_ref.iss(pts, rows, rows, gamma_21=0.45, gamma_32=0.26)['saliency'].all()
    assert not iss_ref.iss(pts, rows, rows, gamma_21=0.45, gamma_32=0.25)['saliency'].any()   # l3 < 0.25 l2 is strict
    # max_nn cuts the rows: the first two columns only -> a segment, l2 = l3 = 0 -> l3 < g l2 fails
    r2 = iss_ref.iss(pts, rows, rows, min_neighbors=2, max_nn=2)
    assert (r2['m'] == 2).all() and not r2['saliency'].any() and np.allclose(r2['eig'][:, 0], 9.0)


def test_summation_runs_in_column_order():
    """1e16 + 1 - 1e16 depends on the order: the restatement follows the row, not the index"""
    pts = np.array([[1e16, 0, 0], [1, 0, 0], [-1e16, 0, 0]], np.float32)
    big = float(np.float32(1e16))
    for row, want in (([0, 1, 2], 0.0), ([0, 2, 1], 1.0), ([1, 0, 2], 0.0)):
        rows = np.tile(np.array(row, np.int32), (3, 1))
        m, Cv = iss_ref.covariance(pts, rows)
        mu = want / 3.0
        d = [{0: big, 1: 1.0, 2: -big}[j] - mu for j in row]
        c00 = 0.0
        for x in d:
            c00 += x * x
        assert Cv[0, 0] == c00 / 3.0


def test_box_corner_yields_a_keypoint_at_the_corner():
    pts = _box_corner()
    rs, rn = 0.15, 0.10
    a, b = iss_ref.radius_rows(pts, rs), iss_ref.radius_rows(pts, rn)
    r = iss_ref.iss(pts, a, b)
    kp = np.flatnonzero(r['mask'])
    assert len(kp) >= 1
    d = np.linalg.norm(pts[kp].astype(np.float64), axis=1)
    assert d.min() < rn, d                                       # a keypoint within the non-max radius of the corner
    # points in the middle of a face are flat: l3 ~ jitter^2, far below the corner's
    mid = np.flatnonzero((np.abs(pts[:, 2]) < 0.01) & (np.abs(pts[:, 0] - 0.3) < 0.06) & (np.abs(pts[:, 1] - 0.3) < 0.06))
    assert len(mid) and not r['mask'][mid].any() and r['eig'][mid, 2].max() < 0.05 * r['eig'][kp[d.argmin()], 2]


def test_isolated_cluster_below_min_neighbors_yields_none():
    rng = np.random.default_rng(1)
    main = rng.random((80, 3))
    far = 10.0 + 0.05 * rng.random((4, 3))                       # four points by themselves: rows of 4 < 5
    pts = np.concatenate([main, far]).astype(np.float32)
    a, b = iss_ref.radius_rows(pts, 0.4), iss_ref.radius_rows(pts, 0.3)
    assert ((a[80:] < 84).sum(1) == 4).all()
    r = iss_ref.iss(pts, a, b)
    assert not r['eig'][80:].any() and not r['saliency'][80:].any() and not r['mask'][80:].any() and r['mask'][:80].any()
    assert iss_ref.iss(pts, a, b, min_neighbors=4)['eig'][80:, 0].all()


def test_doubled_points_come_out_in_pairs():
    pts = np.repeat(np.random.default_rng(0).random((257, 3)).astype(np.float32), 2, 0)
    a, b = iss_ref.radius_rows(pts, 0.3), iss_ref.radius_rows(pts, 0.2)
    assert np.array_equal(a[0::2], a[1::2])                      # twins share their rows (d2 = 0 to each other, then the index)
    r = iss_ref.iss(pts, a, b)
    assert np.array_equal(r['saliency'][0::2], r['saliency'][1::2]) and np.array_equal(r['mask'][0::2], r['mask'][1::2])
    assert int(r['mask'].sum()) == 36 and not r['undecided'].any()


def test_radius_rows_order_and_non_finite_points():
    pts = np.array([[0, 0, 0], [0.3, 0, 0], [0.1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [-0.1, 0, 0]], np.float32)
    rows = iss_ref.radius_rows(pts, 0.35)
    assert rows[0].tolist()[:4] == [0, 2, 5, 1]                 # (d2, index): 2 and 5 tie in d2
    assert (rows[3] == 6).all() and (rows[4] == 6).all() and not np.isin(rows, [3, 4]).any()
    assert iss_ref.radius_rows(pts, 0.35, 2)[0].tolist() == [0, 2]
    two = iss_ref.radius_rows(np.concatenate([pts[:3], pts[:3]]), 0.35, None, [3, 3])
    assert two[:3].max() <= 6 and set(two[:3].ravel()) <= {0, 1, 2, 6} and set(two[3:].ravel()) <= {3, 4, 5, 6}


def test_undecided_points():
    # a point whose l2 sits on gamma_21 l1 is undecided; so is every point with it in its non-max row
    pts = np.array([[3, 0, 0], [-3, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    rows = np.tile(np.arange(6, dtype=np.int32), (6, 1))
    assert iss_ref.iss(pts, rows, rows, gamma_21=4.0 / 9.0)['undecided'].all()
    assert not iss_ref.iss(pts, rows, rows, gamma_21=0.5)['undecided'].any()
    # the same support added in another order: saliencies a few ulp apart -> both undecided
    rng = np.random.default_rng(3)
    p = rng.random((12, 3)).astype(np.float32)
    ra = np.tile(np.arange(12, dtype=np.int32), (12, 1))
    ra[1] = ra[1][::-1]
    r = iss_ref.iss(p, ra, ra)
    if r['saliency'][0] != r['saliency'][1]:
        assert r['undecided'][0] and r['undecided'][1]
    assert iss_ref.MARGIN == 1e-9


def test_keypoints_option(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert a.keypoints == 'all'
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--keypoints', 'iss', '--estimator', 'sc2'])
        assert a.keypoints == 'iss' and a.descriptor == 'fpfh' and a.estimator == 'sc2'
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['--root', 'r', '--keypoints', 'iss'])
        assert e.value.code == 2 and '--keypoints iss' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--keypoints', 'harris'])


def test_ctypes_signature_and_header():
    from buffer_amd import _lib
    assert 'buf_iss_keypoints' in set(_lib.exported_symbols())
    fn = _lib.lib().buf_iss_keypoints
    assert fn.restype is C.c_int
    want = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert list(fn.argtypes) == want
    assert _lib.lib().buf_version() == 670


def test_registration_and_standin_entries():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import fpfh, keypoints
    assert callable(o3d.geometry.keypoint.compute_iss_keypoints) and callable(keypoints.iss_keypoints)
    assert len(o3d.geometry.keypoint.compute_iss_keypoints(o3d.geometry.PointCloud()).points) == 0       # empty in, empty out: no device
    assert fpfh.KEYPOINTS == (None, 'iss')
