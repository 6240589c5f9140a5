"""Generalized ICP on the device (csrc/icp.hip k_icp_correspond<ICP_GICP>, buf_gicp_batched, icp.icp_batched(method='generalized'))
against the float64 restatement tests/gicp_ref.py on its one scene: exact correspondences, one step, the full loop, batch
composition, edge rows and the open3d stand-in.  Kernel and restatement are both fp64 and differ in the order of their sums and in
how they invert a 3x3 / solve the 6x6 system; every tolerance is at most 2 x the printed measurement (tests/util.assert_close)."""
import numpy as np
import pytest
import torch

import gicp_ref
from util import assert_close


def _dev(a, dev):
    return torch.from_numpy(np.array(a, np.float32).reshape(-1, 3)).to(dev)


def _run(dev, src, sn, tgt, tn, **kw):
    from buffer_amd import icp
    kw.setdefault('max_dist', gicp_ref.MAX_DIST)
    max_dist = kw.pop('max_dist')
    return icp.icp_batched([_dev(src, dev)], [_dev(tgt, dev)], max_dist, method='generalized', src_normals=[_dev(sn, dev)],
                           tgt_normals=[_dev(tn, dev)], **kw)[0]


def _scene_run(dev, **kw):
    sc = gicp_ref.scene()
    return _run(dev, sc['src'], sc['src_normals'], sc['tgt'], sc['tgt_normals'], **kw)


def _ref(max_iteration, epsilon=1e-3, init=None, **over):
    sc = dict(gicp_ref.scene(), **over)
    return gicp_ref.icp(sc['src'], sc['tgt'], gicp_ref.MAX_DIST, init, max_iteration, src_normals=sc['src_normals'],
                        tgt_normals=sc['tgt_normals'], epsilon=epsilon)


@pytest.fixture(scope="module", autouse=True)
def before_generalized(dev):
    """point-to-point and point-to-plane results of two pairs, taken before this module makes its first Generalized ICP call (in a
    run of the whole suite no earlier module makes one): test_the_other_methods_keep_their_bits repeats the calls afterwards"""
    from buffer_amd import icp
    sc = gicp_ref.scene()
    S, Tg, N = [_dev(sc['src'], dev), _dev(sc['src'][:257], dev)], [_dev(sc['tgt'], dev), _dev(sc['tgt'][:1500], dev)], \
        [_dev(sc['tgt_normals'], dev), _dev(sc['tgt_normals'][:1500], dev)]
    call = dict(p2p=lambda: icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, max_iteration=40),
                p2l=lambda: icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, method='point_to_plane', tgt_normals=N, max_iteration=40))
    return call, {k: f() for k, f in call.items()}


def _same(a, b):
    return (np.array_equal(a['T'], b['T']) and a['fitness'] == b['fitness'] and a['inlier_rmse'] == b['inlier_rmse']
            and a['iterations'] == b['iterations'])


def _start():
    T0 = np.eye(4)                                                        # a few milliradians / millimetres off the identity
    T0[:3, :3], T0[:3, 3] = gicp_ref.rot(0.004, -0.003, 0.005), [0.004, 0.002, -0.003]
    return T0


# measured on an MI355X, max |T - restatement| after one step: 9.6e-16 (epsilon 1e-3), 1.2e-16 (epsilon 1), 1.4e-15 (start pose off the
# identity); |inlier_rmse - restatement|: 1.0e-17, 1.0e-17, 1.7e-17.  A few units in the last place of fp64: the two differ in the
# order of their sums, the 3x3 inverse (cofactors against LU) and the 6x6 solve (LDL^T against LU).
@pytest.mark.gpu
@pytest.mark.parametrize("name,epsilon,init,atol,atol_rmse", [("eps1e-3", 1e-3, None, 1.9e-15, 2e-17), ("eps1", 1.0, None, 2.4e-16, 2e-17),
                                                             ("start", 1e-3, _start(), 2.7e-15, 3.4e-17)])
def test_zero_iterations_and_one_step_match_the_restatement(dev, name, epsilon, init, atol, atol_rmse):
    sc = gicp_ref.scene()
    inits = None if init is None else [init]
    want0 = _ref(0, epsilon, init)
    r0 = _scene_run(dev, inits=inits, max_iteration=0, epsilon=epsilon, return_correspondences=True)
    assert len(want0['correspondences']) > 600
    assert np.array_equal(r0['correspondences'], want0['correspondences'])          # every brute-force pair, none left out
    assert r0['iterations'] == 0 and np.array_equal(r0['T'], np.eye(4) if init is None else init)
    assert r0['fitness'] == len(want0['correspondences']) / len(sc['src'])
    want1 = _ref(1, epsilon, init)
    r1 = _scene_run(dev, inits=inits, max_iteration=1, epsilon=epsilon, return_correspondences=True)
    assert r1['iterations'] == 1 and want1['iterations'] == 1
    assert_close(r1['T'], want1['T'], 0.0, atol, f'one step T ({name})')
    assert np.array_equal(r1['correspondences'], want1['correspondences'])
    assert_close(r1['inlier_rmse'], want1['inlier_rmse'], 0.0, atol_rmse, f'one step rmse ({name})')


# measured on an MI355X, max |T - restatement| after the loop (3 updates, both): 1.1e-16
@pytest.mark.gpu
def test_full_loop_matches_the_restatement_and_the_planted_pose(dev):
    want = _ref(50)
    r = _scene_run(dev, max_iteration=50, return_correspondences=True)
    assert r['iterations'] == want['iterations'] and 0 < r['iterations'] < 50
    assert_close(r['T'], want['T'], 0.0, 2.2e-16, 'full loop T')
    assert np.array_equal(r['correspondences'], want['correspondences']) and r['fitness'] == want['fitness']
    rot, tr = gicp_ref.pose_error(r['T'], gicp_ref.scene()['T'])
    print(f'device Generalized ICP: {rot:.4f} deg, {tr * 1e3:.3f} mm from the planted pose')
    assert rot < 0.051 and tr < 0.92e-3                                   # the bound tests/test_gicp_cpu.py puts on the restatement


_SIZES = [(0, 1800), (1, 1500), (255, 1700), (256, 1800), (257, 1234), (900, 1800)]


@pytest.mark.gpu
def test_batch_composition_and_reruns_give_the_same_bits(dev):
    from buffer_amd import icp
    sc = gicp_ref.scene()
    S, SN = [_dev(sc['src'][:n], dev) for n, _ in _SIZES], [_dev(sc['src_normals'][:n], dev) for n, _ in _SIZES]
    Tg, TN = [_dev(sc['tgt'][:m], dev) for _, m in _SIZES], [_dev(sc['tgt_normals'][:m], dev) for _, m in _SIZES]
    kw = dict(method='generalized', max_iteration=40)
    a = icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, src_normals=SN, tgt_normals=TN, **kw)
    b = icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, src_normals=SN, tgt_normals=TN, **kw)
    assert all(_same(x, y) for x, y in zip(a, b))
    for i in range(len(_SIZES)):
        one = icp.icp_batched([S[i]], [Tg[i]], gicp_ref.MAX_DIST, src_normals=[SN[i]], tgt_normals=[TN[i]], **kw)[0]
        assert _same(one, a[i]), _SIZES[i]
    rev = icp.icp_batched(S[::-1], Tg[::-1], gicp_ref.MAX_DIST, src_normals=SN[::-1], tgt_normals=TN[::-1], **kw)[::-1]
    assert all(_same(x, y) for x, y in zip(a, rev))
    assert a[0]['iterations'] == 0 and a[0]['fitness'] == 0.0 and np.array_equal(a[0]['T'], np.eye(4))     # empty source
    assert a[1]['iterations'] == 0 and np.array_equal(a[1]['T'], np.eye(4))                                  # one match: no 6x6 system
    assert all(r['iterations'] > 0 and np.isfinite(r['T']).all() for r in a[2:])


@pytest.mark.gpu
def test_the_other_methods_keep_their_bits(dev, before_generalized):
    call, before = before_generalized
    _scene_run(dev, max_iteration=5)
    for k, f in call.items():
        after = f()
        assert all(_same(x, y) for x, y in zip(before[k], after)), k
        assert all(r['iterations'] > 0 for r in after), k


# measured on an MI355X, max |T - restatement| after the loop on the flagged clouds (4 updates, both): 2.2e-16
@pytest.mark.gpu
def test_flagged_rows_are_skipped_and_unusable_normals_count_as_zero(dev):
    sc = gicp_ref.scene()
    src, sn, tn = sc['src'].copy(), sc['src_normals'].copy(), sc['tgt_normals'].copy()
    src[::7] = np.nan
    src[3] = [np.inf, 0, 0]
    sn[1::5] = np.nan                                                     # NaN, non-unit and zero normal rows on both sides
    sn[2::5] *= np.float32(1.5)
    sn[4::10] = 0
    tn[::4] = 0
    tn[1::8] = [np.nan, 0, 1]
    tn[3::8] *= np.float32(0.5)
    tn[5] = [np.inf, 0, 0]
    r = _run(dev, src, sn, sc['tgt'], tn, max_iteration=50, return_correspondences=True)
    bad = np.flatnonzero(~np.isfinite(src).all(1))
    assert np.isfinite(r['T']).all() and r['iterations'] > 0 and r['fitness'] > 0.5
    assert not np.isin(r['correspondences'][:, 0], bad).any()
    want = _ref(50, src=src, src_normals=sn, tgt_normals=tn)
    assert r['iterations'] == want['iterations']
    assert_close(r['T'], want['T'], 0.0, 4.4e-16, 'flagged rows T')
    assert np.array_equal(r['correspondences'], want['correspondences'])
    # normals that all count as zero: the run with zeros in their place, bit for bit
    z = _run(dev, sc['src'], np.zeros_like(sn), sc['tgt'], np.zeros_like(tn), max_iteration=50)
    for junk in (np.nan, 2.0):
        y = _run(dev, sc['src'], np.full_like(sn, junk), sc['tgt'], np.full_like(tn, junk), max_iteration=50)
        assert _same(y, z) and z['iterations'] > 0
    one = _run(dev, sc['src'], sc['src_normals'], sc['tgt'], sc['tgt_normals'], max_iteration=50, epsilon=1.0)
    assert _same(one, z)                                                  # epsilon = 1: the same isotropic steps


@pytest.mark.gpu
def test_few_matches_empty_clouds_and_bad_arguments(dev):
    from buffer_amd import icp
    sc = gicp_ref.scene()
    T0 = np.eye(4)
    T0[:3, 3] = [0.001, 0.0, 0.0]
    S, SN, Tg, TN = (_dev(sc[k], dev) for k in ('src', 'src_normals', 'tgt', 'tgt_normals'))
    T, fit, rmse, corr = icp.icp_generalized(Tg[:5], TN[:5], Tg, TN, 0.003, init=T0)     # 5 exact matches: one short of a 6x6 system
    assert np.array_equal(T, T0) and len(corr) == 5 and fit == 1.0
    for a, an, b, bn in ((S[:0], SN[:0], Tg, TN), (S, SN, Tg[:0], TN[:0])):              # empty source, empty target
        T, fit, rmse, corr = icp.icp_generalized(a, an, b, bn, gicp_ref.MAX_DIST, T0)
        assert np.array_equal(T, T0) and fit == 0.0 and rmse == 0.0 and corr.shape == (0, 2) and corr.dtype == np.int32
    r = icp.icp_batched([S, S[:0]], [Tg[:0], Tg], gicp_ref.MAX_DIST, inits=[T0, T0], method='generalized', src_normals=[SN, SN[:0]],
                        tgt_normals=[TN[:0], TN])
    assert all(np.array_equal(x['T'], T0) and x['fitness'] == 0.0 and x['iterations'] == 0 for x in r)
    for eps in (0.0, -1e-3, 1.5, float('nan')):
        with pytest.raises(ValueError, match="epsilon"):
            icp.icp_generalized(S, SN, Tg, TN, gicp_ref.MAX_DIST, epsilon=eps)
    with pytest.raises(ValueError, match="normals"):
        icp.icp_batched([S], [Tg], gicp_ref.MAX_DIST, method='generalized', tgt_normals=[TN])
    with pytest.raises(ValueError, match="normals"):
        icp.icp_batched([S], [Tg], gicp_ref.MAX_DIST, method='generalized', src_normals=[SN])
    with pytest.raises(ValueError, match="src_normals"):
        icp.icp_batched([S], [Tg], gicp_ref.MAX_DIST, method='generalized', src_normals=[SN[:10]], tgt_normals=[TN])
    with pytest.raises(ValueError, match="tgt_normals"):
        icp.icp_batched([S], [Tg], gicp_ref.MAX_DIST, method='generalized', src_normals=[SN], tgt_normals=[TN, TN])


@pytest.mark.gpu
def test_open3d_standin_generalized_icp(dev):
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import icp
    reg = o3d.pipelines.registration
    sc = gicp_ref.scene()
    pcd0, pcd1 = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
    pcd0.points, pcd1.points = o3d.utility.Vector3dVector(sc['src'].astype(np.float64)), o3d.utility.Vector3dVector(sc['tgt'].astype(np.float64))
    crit = reg.ICPConvergenceCriteria(max_iteration=50)
    bare = reg.registration_generalized_icp(pcd0, pcd1, gicp_ref.MAX_DIST, np.eye(4), reg.TransformationEstimationForGeneralizedICP(), crit)
    assert isinstance(bare, reg.RegistrationResult) and not pcd0.has_normals() and not pcd1.has_normals()
    assert np.isfinite(bare.transformation).all() and bare.fitness > 0.9
    assert len(bare.correspondence_set) == round(bare.fitness * len(sc['src']))
    pcd0.normals, pcd1.normals = (o3d.utility.Vector3dVector(sc[k].astype(np.float64)) for k in ('src_normals', 'tgt_normals'))
    for eps in (1e-3, 0.05):
        res = reg.registration_generalized_icp(pcd0, pcd1, gicp_ref.MAX_DIST, np.eye(4),
                                               reg.TransformationEstimationForGeneralizedICP(epsilon=eps), crit)
        T, fit, rmse, corr = icp.icp_generalized(*(_dev(sc[k], dev) for k in ('src', 'src_normals', 'tgt', 'tgt_normals')),
                                                 gicp_ref.MAX_DIST, np.eye(4), 50, epsilon=eps)
        assert np.array_equal(res.transformation, T) and res.fitness == fit and res.inlier_rmse == rmse
        assert np.array_equal(res.correspondence_set, corr)
    with pytest.raises(NotImplementedError):
        reg.TransformationEstimationForGeneralizedICP(kernel=object())
