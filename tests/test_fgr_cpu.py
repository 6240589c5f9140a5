"""The float64 restatement of N7 (tests/fgr_ref.py) pinned on the CPU: the mixer's known values, the vectorised sampler against a
plain loop, the optimisation against Kabsch on outlier-free rows, the robustness case the GPU test repeats, and the Python surface
that needs no device (exported symbols, the drivers' --estimator)."""
import numpy as np
import pytest

import fgr_cases
import fgr_ref


def test_splitmix64_known_values():
    assert fgr_ref.splitmix64(0) == 0xE220A8397B1DCDAF and fgr_ref.splitmix64(1) == 0x910A2DEC89025CC1
    got = fgr_ref.splitmix64_np(np.array([0, 1, (1 << 64) - 1], np.uint64))
    assert [int(v) for v in got] == [fgr_ref.splitmix64(0), fgr_ref.splitmix64(1), fgr_ref.splitmix64((1 << 64) - 1)]


@pytest.mark.parametrize('n,max_tuples,scale', [(7, 1000, 0.95), (40, 5, 0.95), (40, 1000, 0.9999), (3, 1000, 0.95)])
def test_vectorised_sampler_equals_the_sequential_loop(n, max_tuples, scale):
    src, tgt, _ = fgr_cases.moved_cloud(3, 40, 0.001)
    corr = np.stack([np.arange(n), np.arange(n)], 1)
    for seed in (0, 5, (1 << 64) - 2):                           # the last one wraps seed + 3 t + k
        a = fgr_ref.tuples(src, tgt, corr, seed, scale, max_tuples, 100)
        b = fgr_ref.tuples_sequential(src, tgt, corr, seed, scale, max_tuples, 100)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (a[1:], b[1:])
    if max_tuples == 5:
        assert a[1] == 5 and a[2] < 100 * n and (a[0][:15] >= 0).all() and (a[0][15:] == -1).all()      # the cap was reached
    if scale == 0.9999:
        assert a[1] < max_tuples and a[2] == 100 * n                                                     # the budget ran out


def test_rejections():
    src, tgt, _ = fgr_cases.moved_cloud(3, 40)
    same = np.zeros((20, 2), np.int64)                           # one correspondence repeated: every edge is 0, nothing passes
    assert fgr_ref.tuples(src, tgt, same, 1)[1:] == (0, 2000)
    corr = np.stack([np.arange(12), np.arange(12)], 1)
    base = fgr_ref.tuples(src, tgt, corr, 1)
    bad = corr.copy()
    bad[4, 1] = 40                                               # an index outside the target cloud
    nanp = src.copy()
    nanp[7, 1] = np.nan
    for s, c, row in ((src, bad, 4), (nanp, corr, 7)):
        got = fgr_ref.tuples(s, tgt, c, 1)
        assert got[1] < base[1] and not (got[0][:3 * got[1], 0] == row).any()
        assert np.array_equal(got[0], fgr_ref.tuples_sequential(s, tgt, c, 1)[0])
    assert fgr_ref.tuples(src, tgt, np.zeros((0, 2), np.int64), 1)[1:] == (0, 0)


def test_outlier_free_rows_give_the_kabsch_pose():
    src, tgt, _ = fgr_cases.moved_cloud(8, 200)
    corr = np.stack([np.arange(200), np.arange(200)], 1)
    out = fgr_ref.fgr(src, tgt, corr, 2)
    assert out['info'][0] == fgr_ref.OK and out['info'][1] == 1000 and out['info'][3] == 64
    rows = out['rows']
    ref = fgr_cases.kabsch64(src[rows[:, 0]], tgt[rows[:, 1]])    # over the kept rows: what the weighted least squares minimises
    # the residuals are the fp32 rounding of the target (1e-8 relative): every weight is 1 to 1e-13, so the minimiser is Kabsch's
    assert np.abs(out['T'] - ref).max() <= 1e-10, np.abs(out['T'] - ref).max()
    assert np.nanmin(out['weights']) > 1 - 1e-9 and np.isnan(out['weights']).sum() == 0


def test_statuses():
    src, tgt, _ = fgr_cases.moved_cloud(8, 200)
    corr = np.stack([np.arange(200), np.arange(200)], 1)
    few = fgr_ref.fgr(src, tgt, corr, 2, max_tuples=3)           # 9 rows
    assert few['info'].tolist()[:2] == [fgr_ref.NOTHING, 3] and few['info'][3] == 0 and np.array_equal(few['T'], np.eye(4))
    assert np.isnan(few['weights']).all()
    assert fgr_ref.fgr(src, tgt, corr, 2, max_tuples=4)['info'][0] == fgr_ref.OK                         # 12 rows
    zero = fgr_ref.fgr(src, tgt, corr, 2, iterations=0)
    assert zero['info'].tolist()[0] == fgr_ref.OK and zero['info'][3] == 0 and np.array_equal(zero['T'], np.eye(4))
    one = np.tile(src[:1], (50, 1))                              # clouds of one repeated point: D == 0
    assert fgr_ref.fgr(one, one, corr[:50], 2)['info'].tolist() == [fgr_ref.NOTHING, 0, 5000, 0]
    # points on the x axis with exact arithmetic: the rotation about the axis is unobservable, H[0][0] == 0 exactly
    line = np.zeros((9, 3), np.float32)
    line[:, 0] = np.arange(-4, 5) / 4.0
    c9 = np.stack([np.arange(9), np.arange(9)], 1)
    out = fgr_ref.fgr(line, line, c9, 2)
    assert out['info'][0] == fgr_ref.FAILED and out['info'][1] >= 4 and out['info'][3] == 0 and np.array_equal(out['T'], np.eye(4))
    assert (out['weights'][:3 * out['info'][1]] == 1.0).all()    # the failed linearisation's weights


@pytest.mark.parametrize('case', range(4))
def test_robustness_case(case):
    """half the rows false: the line process recovers the pose, plain least squares over all rows does not"""
    for variant, lim in ((False, (0.5, 0.01)), (True, (0.5, 0.01))):
        src, tgt, corr, T, seed = fgr_cases.robust_case(case, variant)
        out = fgr_ref.fgr(src, tgt, corr, seed)
        rre, rte = fgr_cases.errors(out['T'], T)
        kept = out['rows'][:3 * out['info'][1]]
        false = float((kept[:, 0] >= 150).mean())
        print(f'FGR restatement case {case} variant {variant}: info {out["info"].tolist()}, false rows kept {false:.4f}, '
              f'{rre:.3e} deg, {rte:.3e}')
        assert out['info'][0] == fgr_ref.OK and rre <= lim[0] and rte <= lim[1]
        if not variant:
            assert fgr_cases.errors(fgr_cases.kabsch64(src[corr[:, 0]], tgt[corr[:, 1]]), T)[0] > 5.0
            assert out['info'][1] == 1000


def test_options_map_onto_the_kernel_arguments():
    from buffer_amd.fgr import FgrOptions
    o = FgrOptions()
    assert (o.division_factor, o.use_absolute_scale, o.decrease_mu, o.maximum_correspondence_distance, o.iteration_number, o.tuple_scale,
            o.maximum_tuple_count) == (1.4, False, True, 0.025, 64, 0.95, 1000)
    assert o.kernel_arguments() == dict(tuple_scale=0.95, max_tuples=1000, trial_factor=100, mu_start=1.0, delta=0.025, delta_absolute=False,
                                        division_factor=1.4, decrease_every=4, iterations=64)
    k = FgrOptions(decrease_mu=False).kernel_arguments()
    assert k['delta'] > 1e300 and np.isfinite(k['delta']) and not k['delta_absolute']      # mu > floor never holds
    with pytest.raises(NotImplementedError):
        FgrOptions(use_absolute_scale=True).kernel_arguments()


def test_standin_declares_the_entry():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    regm = o3d.pipelines.registration
    o = regm.FastGlobalRegistrationOption()
    assert (o.division_factor, o.use_absolute_scale, o.decrease_mu, o.maximum_correspondence_distance, o.iteration_number, o.tuple_scale,
            o.maximum_tuple_count) == (1.4, False, True, 0.025, 64, 0.95, 1000)
    assert callable(regm.registration_fast_based_on_feature_matching)


def test_estimator_option(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh'])
        assert a.estimator == 'ransac'
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--estimator', 'fgr'])
        assert a.descriptor == 'fpfh' and a.estimator == 'fgr'
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['--root', 'r', '--estimator', 'fgr'])
        assert e.value.code == 2 and '--descriptor fpfh' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--estimator', 'teaser'])
    from buffer_amd.fpfh import ESTIMATORS
    assert ESTIMATORS == ('ransac', 'fgr')


def test_header_declares_the_entry_points():
    from buffer_amd import _lib
    assert {'buf_fgr_batched', 'buf_fgr_ws_bytes'} <= set(_lib.exported_symbols())
