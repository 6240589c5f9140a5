"""The outlier filters, the resolution estimate and the one-pass k-NN normals (preprocess.py on N14 / N15) against float64:
tests/knn3_ref.py restates the statistical rule; the radius filter is checked against all-pairs counts."""
import numpy as np
import pytest
import torch

import knn3_ref

pytestmark = pytest.mark.gpu


def plane_scene(seed):
    """a 1 m x 1 m plane patch of 600 points (sigma 2 mm) and 12 planted points 0.3 - 0.8 off it -> (f32[612,3], planted rows)"""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.random((600, 2)), rng.normal(0.0, 0.002, (600, 1))], 1)
    far = np.concatenate([rng.random((12, 2)), rng.uniform(0.3, 0.8, (12, 1)) * rng.choice([-1.0, 1.0], (12, 1))], 1)
    pts = np.concatenate([p, far]).astype(np.float32)
    perm = rng.permutation(612)
    return pts[perm], np.flatnonzero(perm >= 600)


def gradient_scene(seed):
    """800 points whose density falls along x (exponential, scale 0.5) in a 1 x 1 cross-section: the threshold cuts a continuum"""
    rng = np.random.default_rng(100 + seed)
    return np.concatenate([rng.exponential(0.5, (800, 1)), rng.random((800, 2))], 1).astype(np.float32)


def _reference(pts, lens, nb, ratio):
    _, d2 = knn3_ref.brute_force(pts, pts, lens, lens, nb)
    return knn3_ref.statistical(d2, lens, ratio)


def _guard(mean, stats, lens):
    """the test's own guard: no mean_i within 1e-9 thr of its cloud's thr -> the smallest relative distance"""
    lo, closest = 0, np.inf
    for c, m in enumerate(lens):
        thr = stats[c, 2]
        if m and np.isfinite(thr):
            gap = np.abs(mean[lo:lo + m] - thr).min() / thr
            assert gap > 1e-9, (c, gap)
            closest = min(closest, gap)
        lo += m
    return closest


def _check(pts, lens, nb, ratio, dev, guard=True):
    from buffer_amd import preprocess
    want_mean, want_stats, want_keep = _reference(pts, lens, nb, ratio)
    closest = _guard(want_mean, want_stats, lens) if guard else None
    keep, new_lens, mean, stats = preprocess.remove_statistical_outlier(torch.from_numpy(pts).to(dev), nb, ratio, lengths=lens)
    assert keep.dtype == torch.bool and mean.dtype == torch.float64 and stats.shape == (len(lens), 3)
    assert isinstance(new_lens, np.ndarray) and new_lens.dtype == np.int32
    mean, stats, keep = mean.cpu().numpy(), stats.cpu().numpy(), keep.cpu().numpy()
    assert np.array_equal(mean.view(np.uint64), want_mean.view(np.uint64))
    print('stats', stats.tolist(), 'reference', want_stats.tolist(), 'closest mean_i to thr (relative)', closest)
    fin = np.isfinite(want_stats)
    assert np.array_equal(fin, np.isfinite(stats))
    assert np.allclose(stats[fin], want_stats[fin], rtol=1e-12, atol=0.0)
    assert np.array_equal(keep, want_keep)
    offs = np.concatenate([[0], np.cumsum(lens)])
    assert np.array_equal(new_lens, [int(want_keep[offs[c]:offs[c + 1]].sum()) for c in range(len(lens))])
    return want_keep, closest


def test_planted_points_off_a_plane(dev):
    scenes = [plane_scene(s) for s in range(4)]
    pts = np.concatenate([p for p, _ in scenes])
    lens = [612] * 4
    keep, _ = _check(pts, lens, 20, 2.0, dev)
    for c, (_, planted) in enumerate(scenes):
        k = keep[612 * c:612 * (c + 1)]
        assert not k[planted].any() and int((~k).sum()) == 12    # all 12 planted points go, no point of the plane does


def test_threshold_through_a_density_gradient(dev):
    from buffer_amd import preprocess
    scenes = [gradient_scene(s) for s in range(6)]
    pts, lens = np.concatenate(scenes), [800] * 6
    keep, closest = _check(pts, lens, 16, 1.0, dev)
    removed = [int((~keep[800 * c:800 * (c + 1)]).sum()) for c in range(6)]
    print('removed per cloud', removed)
    # a guard on the scene (reference values): the threshold cuts through the continuum, 46 - 70 of 800 go (the float64 restatement on the
    # CPU: 48, 53, 58, 46, 68, 70; the closest mean_i lies 1.5e-4 thr from thr)
    assert removed == [48, 53, 58, 46, 68, 70] and closest < 1e-3
    # a cloud's numbers are the same bits alone or stacked
    t = torch.from_numpy(pts).to(dev)
    all_ = preprocess.remove_statistical_outlier(t, 16, 1.0, lengths=lens)
    for c in (0, 5):
        one = preprocess.remove_statistical_outlier(t[800 * c:800 * (c + 1)], 16, 1.0)
        assert torch.equal(one[0], all_[0][800 * c:800 * (c + 1)]) and int(one[1][0]) == int(all_[1][c])
        assert torch.equal(one[2].view(torch.int64), all_[2][800 * c:800 * (c + 1)].view(torch.int64))
        assert torch.equal(one[3].view(torch.int64), all_[3][c:c + 1].view(torch.int64))


def test_tiny_clouds_and_more_neighbours_than_points(dev):
    from buffer_amd import preprocess
    rng = np.random.default_rng(7)
    pts = rng.random((0 + 1 + 2 + 9, 3)).astype(np.float32)
    lens = [0, 1, 2, 9]
    # k = 20 > n everywhere: padded rows.  (No guard: in the two-point cloud both means EQUAL thr, exactly and by the rule -- mu = (m + m) / 2
    # = m, every deviation is 0, sd = 0 -- so the strict < is decided without rounding.)
    keep, _ = _check(pts, lens, 20, 2.0, dev, guard=False)
    assert not keep[:3].any()                                    # the rule, literally: one and two points keep nothing
    k2, l2, mean, stats = preprocess.remove_statistical_outlier(torch.from_numpy(pts).to(dev), 20, 2.0, lengths=lens)
    stats = stats.cpu().numpy()
    assert np.isnan(stats[0, [0, 2]]).all() and stats[0, 1] == 0.0          # no rows: mu = 0 / 0, sd = sqrt(0 / -1) = -0
    assert stats[1, 0] == 0.0 and np.isnan(stats[1, 1]) and stats[2, 1] == 0.0 and stats[2, 2] == stats[2, 0]
    assert l2.tolist()[:3] == [0, 0, 0] and float(mean[0]) == 0.0
    e = preprocess.remove_statistical_outlier(torch.zeros((0, 3), device=dev), 5, 1.0)
    assert e[0].shape == (0,) and e[1].tolist() == [0] and e[2].shape == (0,)


def test_radius_filter_against_all_pairs_counts(dev):
    from buffer_amd import preprocess
    rng = np.random.default_rng(8)
    a = rng.random((400, 3)).astype(np.float32)
    # a row of points exactly r = 0.25 apart (0.25 and its multiples are exact in fp32): d2 == r * r is outside the ball
    b = np.zeros((6, 3), np.float32)
    b[:, 0] = 0.25 * np.arange(6)
    pts, lens, r = np.concatenate([a, b + 5.0]), [400, 6], 0.25
    d2a, d2b = knn3_ref.sqdist3(a, a), knn3_ref.sqdist3(b + 5.0, b + 5.0)
    r2 = np.float32(r) * np.float32(r)
    counts = np.concatenate([(d2a < r2).sum(1), (d2b < r2).sum(1)])
    assert (counts[400:] == 1).all() and (d2b == r2).sum() == 10
    for nb in (0, 1, 20, 30):
        keep, new_lens = preprocess.remove_radius_outlier(torch.from_numpy(pts).to(dev), nb, r, lengths=lens)
        want = counts > nb
        assert np.array_equal(keep.cpu().numpy(), want) and new_lens.tolist() == [int(want[:400].sum()), int(want[400:].sum())]
        assert new_lens.dtype == np.int32 and keep.dtype == torch.bool


def test_nearest_neighbor_distance_and_resolution(dev):
    from buffer_amd import preprocess
    rng = np.random.default_rng(9)
    a = rng.random((300, 3)).astype(np.float32)
    a[10] = a[3]                                                 # a duplicate: distance 0 on both
    a[200] = a[100]
    pts, lens = np.concatenate([a, a[:1], rng.random((50, 3)).astype(np.float32)]), [300, 1, 50]
    want = np.concatenate([np.sqrt(np.sort(knn3_ref.sqdist3(c, c), axis=1)[:, 1:2].astype(np.float64)).ravel() if len(c) > 1
                           else np.full(len(c), np.inf) for c in (pts[:300], pts[300:301], pts[301:])])
    got = preprocess.nearest_neighbor_distance(torch.from_numpy(pts).to(dev), lens)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)
    assert want[3] == 0 and want[10] == 0 and want[100] == 0 and np.isinf(want[300])
    res = preprocess.cloud_resolution(torch.from_numpy(pts).to(dev), lens).cpu().numpy()
    assert np.allclose([res[0], res[2]], [want[:300].mean(), want[301:].mean()], rtol=1e-12) and np.isnan(res[1])


def test_knn_search_and_knn_normals(dev):
    from buffer_amd import ops, preprocess
    rng = np.random.default_rng(10)
    a = np.concatenate([rng.random((500, 2)), 0.01 * rng.normal(size=(500, 1))], 1).astype(np.float32)
    b = (rng.random((40, 3)) + 2.0).astype(np.float32)
    pts, lens = np.concatenate([a, b]), [500, 40]
    t = torch.from_numpy(pts).to(dev)
    want_nbr, want_d2 = knn3_ref.brute_force(pts, pts, lens, lens, 30)
    for kw in (dict(), dict(cell=0.3), dict(grid=ops.CellGrid(t, lens, 0.05))):
        idx, d2 = preprocess.knn_search(t, 30, lens, **kw)
        assert np.array_equal(idx.cpu().numpy(), want_nbr) and np.array_equal(d2.cpu().numpy().view(np.uint32), want_d2.view(np.uint32))
    rows = torch.from_numpy(want_nbr).to(dev)
    cam = (0.5, 0.5, 3.0)
    nrm, cov = preprocess.estimate_normals_knn(t, 30, cam, lengths=lens, return_cov=True)
    w_nrm, w_cov = ops.row_normals(t, rows, 0, cam, return_cov=True)
    assert torch.equal(nrm, w_nrm) and torch.equal(cov, w_cov)
    assert torch.equal(preprocess.estimate_normals_knn(t, 30, orient=False, lengths=lens), ops.row_normals(t, rows, 0, None))
    assert float(nrm[:500, 2].abs().median()) > 0.95             # the plane's normal
    assert preprocess.estimate_normals_knn(t[:0], 30).shape == (0, 3)


def test_iss_radii_from_the_estimated_resolution(dev):
    from buffer_amd import fpfh, preprocess
    from buffer_amd.config import THREEDMATCH
    from test_fpfh_register_gpu import _upload
    from test_iss_register_gpu import _pair
    p, ref, _ = _pair(11, 0.7)
    inp = _upload(p, dev)
    base = fpfh.FpfhRegistration(THREEDMATCH, dev, keypoints='iss')
    same = fpfh.FpfhRegistration(THREEDMATCH, dev, keypoints='iss', iss_resolution='voxel')
    assert base.iss_resolution == 'voxel'
    a, b = base.register_batch([inp], [3]), same.register_batch([inp], [3])
    assert torch.equal(a[0], b[0]) and np.array_equal(base.keypoint_counts, same.keypoint_counts)
    assert base.iss_radii == (6.0 * THREEDMATCH.voxel_size_0, 4.0 * THREEDMATCH.voxel_size_0)     # the radii as they were
    est = fpfh.FpfhRegistration(THREEDMATCH, dev, keypoints='iss', iss_resolution='estimate')
    pose = est.register_batch([inp], [3])[0]
    res = float(preprocess.cloud_resolution(inp['points'], inp['lengths']).mean())
    # (the mean of two numbers, taken here and there by different reductions: equal up to the rounding of one addition)
    assert est.iss_radii == pytest.approx((6.0 * res, 4.0 * res), rel=1e-14) and 0.0 < res < THREEDMATCH.voxel_size_0 * 4
    assert pose.shape == (4, 4) and bool(torch.isfinite(pose).all()) and (est.keypoint_counts > 0).all()
    print('iss_resolution=estimate: resolution', res, 'radii', est.iss_radii, 'keypoints', est.keypoint_counts.tolist())
    with pytest.raises(ValueError, match='unknown iss_resolution'):
        fpfh.FpfhRegistration(THREEDMATCH, dev, iss_resolution='guess')
