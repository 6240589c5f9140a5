"""The float64 restatement of the FPFH contract (tests/fpfh_ref.py) pinned on hand cases, and the host-side pieces of the baseline:
the open3d stand-in's Feature, the numpy twin of fpfh.match, the --descriptor option.  No device."""
import math

import numpy as np
import pytest

import fpfh_ref


def _rows(n, rows, k=4):
    out = np.full((n, k), n, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def test_two_points_by_hand():
    pts = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    assert fpfh_ref.pair_feature((0., 0., 0.), (0., 0., 1.), (1., 0., 0.), (0., 0., 1.)) == (0.0, 0.0, 0.0)
    spfh, out, margin = fpfh_ref.fpfh(pts, nrm, _rows(2, [[0, 1], [1, 0]]), 100)
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(spfh[0], want) and np.array_equal(spfh[1], want)
    # acc = spfh[j] / 1 -> each block sums to 100 and is scaled by 1; + the point's own SPFH
    assert np.array_equal(out[0], 2 * want) and np.array_equal(out[0], out[1])
    assert abs(margin - 0.5) < 1e-12
    assert np.array_equal(fpfh_ref.radius_rows(pts, 1.5, 4), _rows(2, [[0, 1], [1, 0]]))


def test_rows_shorter_than_two_are_zero_and_max_nn_truncates():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))
    spfh, out, _ = fpfh_ref.fpfh(pts, nrm, _rows(3, [[0, 1, 2], [1, 0, 2], [2]]), 100)
    assert not spfh[2].any() and not out[2].any()
    assert spfh[0, 5] == 100.0 and spfh[0].sum() == 300.0                  # two pairs, 50 each, same bins
    s2, o2, _ = fpfh_ref.fpfh(pts, nrm, _rows(3, [[0, 1, 2], [1, 0, 2], [2]]), 2)
    s1, o1, _ = fpfh_ref.fpfh(pts, nrm, _rows(3, [[0, 1], [1, 0], [2]], k=2), 100)
    assert np.array_equal(s2, s1) and np.array_equal(o2, o1)


def test_block_sums():
    rng = np.random.default_rng(0)
    pts = rng.random((64, 3)).astype(np.float32)
    nrm = rng.normal(size=(64, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nbr = fpfh_ref.radius_rows(pts, 0.3, 100)
    spfh, out, margin = fpfh_ref.fpfh(pts, nrm, nbr, 100)
    m = (nbr < 64).sum(1)
    assert (m >= 2).any() and margin > 0
    for i in range(64):
        bs, bf = spfh[i].reshape(3, 11).sum(1), out[i].reshape(3, 11).sum(1)
        if m[i] < 2:
            assert not spfh[i].any() and not out[i].any()
            continue
        assert np.abs(bs - 100.0).max() < 1e-12
        assert np.abs(bf - 200.0).max() < 1e-12          # (radius rows are symmetric: every neighbour has a non-empty SPFH)


def test_swap_branch_both_ways():
    """n_i = z, n_j = (0.6, 0, 0.8), d = x: seen from i, |a1| = 0 < |a2| = 0.6 swaps; seen from j, |a1| = 0.6 > |a2| = 0 does not:
    both give the frame of n_j and the same feature"""
    pi, ni = (0., 0., 0.), (0., 0., 1.)
    pj, nj = (1., 0., 0.), (float(np.float32(0.6)), 0., float(np.float32(0.8)))
    fi = fpfh_ref.pair_feature(pi, ni, pj, nj)
    fj = fpfh_ref.pair_feature(pj, nj, pi, ni)
    want = (math.atan2(0.6, 0.8), 0.0, -0.6)
    for f in (fi, fj):
        assert max(abs(a - b) for a, b in zip(f, want)) < 1e-7
    assert fi[2] == -nj[0] and fj[2] == -nj[0]
    x = fpfh_ref.bin_coordinates(fi)
    assert [fpfh_ref._bin(v) for v in x] == [6, 5, 2]
    spfh, _, _ = fpfh_ref.fpfh(np.array([pi, pj], np.float32), np.array([ni, nj], np.float32), _rows(2, [[0, 1], [1, 0]]), 100)
    want_row = np.zeros(33)
    want_row[[6, 16, 24]] = 100.0
    assert np.array_equal(spfh[0], want_row) and np.array_equal(spfh[1], want_row)


def test_zero_cross_product_gives_the_zero_feature():
    """n_j = d: the swap makes n1 parallel to d, v = d x n1 = 0 -> f = (0, 0, 0), f2 included (it was -1 before)"""
    assert fpfh_ref.pair_feature((0., 0., 0.), (0., 0., 1.), (1., 0., 0.), (1., 0., 0.)) == (0.0, 0.0, 0.0)
    # without the swap: n_i parallel to d
    assert fpfh_ref.pair_feature((0., 0., 0.), (1., 0., 0.), (2., 0., 0.), (0., 0., 1.)) == (0.0, 0.0, 0.0)


def test_duplicate_point_is_binned_but_carries_no_weight():
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8]], np.float32)
    nbr = _rows(3, [[0, 1, 2], [1, 0, 2], [2, 0, 1]])
    spfh, out, _ = fpfh_ref.fpfh(pts, nrm, nbr, 100)
    assert spfh[0, 5] >= 50.0 and spfh[0, 16] >= 50.0 and spfh[0, 27] >= 50.0       # the pair (0, 1) has L = 0: the zero feature, counted
    assert abs(spfh[0].sum() - 300.0) < 1e-12
    # FPFH of point 0: neighbour 1 (d2 = 0) is skipped, neighbour 2 has weight 1 and block sums of 100 -> scale 1
    assert np.array_equal(out[0], spfh[2] + spfh[0])
    assert np.array_equal(out[1], spfh[2] + spfh[1])


def test_nan_goes_to_bin_zero():
    pts = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nbr = _rows(2, [[0, 1], [1, 0]])
    nan = float('nan')
    spfh, out, margin = fpfh_ref.fpfh(pts, np.array([[nan, 0, 1], [0, 0, 1]], np.float32), nbr, 100)
    want = np.zeros(33)
    want[[0, 11, 22]] = 100.0                                  # n_i NaN: a1, v and every feature are NaN
    assert np.array_equal(spfh[0], want)
    # seen from point 1 the NaN normal is n_j: |a1| < NaN is false, f2 = a1 = 0 stays finite, f0 and f1 are NaN
    want1 = np.zeros(33)
    want1[[0, 11, 27]] = 100.0
    assert np.array_equal(spfh[1], want1)
    assert np.isfinite(out).all() and abs(margin - 0.5) < 1e-12
    assert fpfh_ref._bin(nan) == 0 and fpfh_ref._bin(-math.inf) == 0 and fpfh_ref._bin(math.inf) == 10 and fpfh_ref._bin(11.0) == 10
    assert fpfh_ref._bin(10.999) == 10 and fpfh_ref._bin(0.0) == 0 and fpfh_ref._bin(-1e-300) == 0


def test_margin_is_the_distance_to_the_nearest_bin_edge():
    f = (0.0, 2.0 / 11.0 * 1.001 - 1.0, 0.0)                 # x1 just above 1
    x = fpfh_ref.bin_coordinates(f)
    assert abs(x[1] - 1.001) < 1e-12 and fpfh_ref._bin(x[1]) == 1


def test_standin_feature_shapes():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    reg = o3d.pipelines.registration
    f = reg.Feature()
    assert f.dimension() == 0 and f.num() == 0
    f.data = np.zeros((33, 7))
    assert f.dimension() == 33 and f.num() == 7 and f.data.dtype == np.float64
    f.resize(33, 5)
    assert f.data.shape == (33, 5)
    assert hasattr(reg, 'compute_fpfh_feature') and hasattr(reg, 'registration_ransac_based_on_feature_matching')
    pcd = o3d.geometry.PointCloud(np.zeros((4, 3)))
    with pytest.raises(RuntimeError):                                            # no normals
        reg.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(0.1, 100))
    pcd.normals = np.tile([[0., 0., 1.]], (4, 1))
    for param in (o3d.geometry.KDTreeSearchParamKNN(30), o3d.geometry.KDTreeSearchParamRadius(0.1)):
        with pytest.raises(NotImplementedError):
            reg.compute_fpfh_feature(pcd, param)


def test_match_twin_on_a_hand_matrix():
    fa = np.array([[0.0, 0.0], [10.0, 0.0], [0.1, 0.0], [5.0, 5.0]])
    fb = np.array([[10.0, 0.1], [0.0, 0.0], [5.0, 6.0]])
    # a -> b: 0 -> 1, 1 -> 0, 2 -> 1, 3 -> 2; b -> a: 0 -> 1, 1 -> 0, 2 -> 3
    assert fpfh_ref.match(fa, fb, mutual=False).tolist() == [[0, 1], [1, 0], [2, 1], [3, 2]]
    assert fpfh_ref.match(fa, fb, mutual=True).tolist() == [[0, 1], [1, 0], [3, 2]]
    assert fpfh_ref.match(fa[:0], fb).shape == (0, 2) and fpfh_ref.match(fa, fb).dtype == np.int32
    # ties go to the lowest row
    assert fpfh_ref.match(np.zeros((1, 2)), np.zeros((3, 2)), mutual=False).tolist() == [[0, 0]]


def test_descriptor_option(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert a.descriptor == 'buffer'
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--refine', 'point_to_plane'])
        assert a.descriptor == 'fpfh' and a.refine == 'point_to_plane'
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--stage-metrics'])
        assert e.value.code == 2 and '--stage-metrics' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--descriptor', 'sift'])


def test_header_declares_the_entry_points():
    from buffer_amd import _lib
    assert {'buf_fpfh', 'buf_fpfh_ws_bytes'} <= set(_lib.exported_symbols())
