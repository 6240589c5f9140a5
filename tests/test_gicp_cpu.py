"""Generalized ICP, the parts that need no device: the float64 restatement (tests/gicp_ref.py) pinned on its scene, the C ABI of
buf_gicp_batched (argument checks come before any device call), the Python argument checks and the open3d stand-in's class."""
import ctypes as C
import math

import numpy as np
import pytest

import gicp_ref


@pytest.fixture(scope="module")
def lib():
    from buffer_amd import _lib, build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def runs():
    """the restatement from the identity, 50 iterations at most: Generalized ICP at epsilon 1e-3 and 1, with all-zero normals, and the
    Kabsch point-to-point loop; the last three also with the relative criteria off (they then run to their fixed point)"""
    sc = gicp_ref.scene()
    zero = dict(src_normals=np.zeros_like(sc['src_normals']), tgt_normals=np.zeros_like(sc['tgt_normals']))
    nrm = dict(src_normals=sc['src_normals'], tgt_normals=sc['tgt_normals'])
    off = dict(relative_fitness=0.0, relative_rmse=0.0)

    def run(**kw):
        return gicp_ref.icp(sc['src'], sc['tgt'], gicp_ref.MAX_DIST, None, 50, **kw)
    return dict(gicp=run(epsilon=1e-3, **nrm), eps1=run(epsilon=1.0, **nrm), zero=run(epsilon=1e-3, **zero),
                p2p=run(method='point_to_point'), eps1_fixed=run(epsilon=1.0, **nrm, **off), zero_fixed=run(epsilon=1e-3, **zero, **off),
                p2p_fixed=run(method='point_to_point', **off))


def test_scene_is_the_one_written_down():
    sc = gicp_ref.scene()
    assert sc['src'].shape == (900, 3) and sc['tgt'].shape == (1800, 3) and sc['src'].dtype == np.float32
    assert np.array_equal(np.abs(sc['tgt_normals']).sum(1), np.ones(1800))           # analytic: a coordinate axis each
    assert np.abs((sc['src_normals'].astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6
    R, t = sc['T'][:3, :3], sc['T'][:3, 3]
    on = sc['src'].astype(np.float64) @ R.T + t                                      # the planted pose puts the source on the walls
    assert np.abs(on).min(1).max() < 6 * gicp_ref.SIGMA and on.min() > -6 * gicp_ref.SIGMA and on.max() < 1 + 1e-6


def test_restatement_converges_and_beats_point_to_point(runs):
    """Measured with this file: Generalized ICP 0.0254 deg / 0.46 mm after 3 updates, point-to-point 0.626 deg / 11.6 mm after 27
    (ratios 24.6 / 25.1).  The bounds on the Generalized ICP pose are 2 x its own figures: a condition on the inputs."""
    T = gicp_ref.scene()['T']
    g, p = runs['gicp'], runs['p2p']
    (gr, gt), (pr, pt) = gicp_ref.pose_error(g['T'], T), gicp_ref.pose_error(p['T'], T)
    print(f'generalized {gr:.4f} deg {gt * 1e3:.3f} mm in {g["iterations"]}; point-to-point {pr:.4f} deg {pt * 1e3:.3f} mm in {p["iterations"]}')
    assert 0 < g['iterations'] < 50 and 0 < p['iterations'] < 50                     # both stop on the relative criteria
    assert g['fitness'] == 1.0
    assert gr < 0.051 and gt < 0.92e-3
    assert 3 * gr <= pr and 3 * gt <= pt


def test_unit_epsilon_and_zero_normals_end_at_the_point_to_point_fixed_point(runs):
    """epsilon = 1 makes every covariance the identity and so do normals taken as zero: M = (I + R R^T)^-1, the Gauss-Newton step of
    the point-to-point objective.  The two runs are the same arithmetic (w = 0 against n = 0: the same bits).  With the relative
    criteria off both, and the Kabsch loop, stop moving at the pose where the update of the current matches is the identity; what
    is left between them is fp64 rounding of sums over 900 matches through a 6x6 system of condition ~1e2: 900 * 2.2e-16 * 1e2 =
    2e-11 (measured 2.3e-15)."""
    assert np.array_equal(runs['eps1']['T'], runs['zero']['T']) and runs['eps1']['iterations'] == runs['zero']['iterations']
    assert np.array_equal(runs['eps1_fixed']['T'], runs['zero_fixed']['T'])
    d = np.abs(runs['eps1_fixed']['T'] - runs['p2p_fixed']['T']).max()
    print(f'Gauss-Newton vs Kabsch fixed point: {d:.3g}')
    assert d < 2e-11
    assert np.array_equal(runs['eps1_fixed']['correspondences'], runs['p2p_fixed']['correspondences'])
    # under the default criteria the loops stop a little short of it, each where its rmse moved by less than 1e-6
    assert np.abs(runs['eps1']['T'] - runs['p2p_fixed']['T']).max() < 1e-5


def test_restatement_edges():
    sc = gicp_ref.scene()
    n = sc['tgt_normals'].copy()
    n[0], n[1], n[2], n[3] = [np.nan, 0, 1], [0, 0, 1.01], [0, 0, 0], [np.inf, 0, 0]
    u = gicp_ref.usable_normals(n)
    assert np.array_equal(u[:4], np.zeros((4, 3))) and np.array_equal(u[4:], n[4:].astype(np.float64))
    q = sc['src'][:4].copy()
    q[1, 0] = np.nan
    nn = gicp_ref.brute_nn(q, q, 0.1)
    assert nn.tolist() == [0, -1, 2, 3]
    r = gicp_ref.icp(sc['tgt'][:5], sc['tgt'], src_normals=sc['tgt_normals'][:5], tgt_normals=sc['tgt_normals'])
    assert r['iterations'] == 0 and np.array_equal(r['T'], np.eye(4)) and len(r['correspondences']) == 5


# ---------------------------------------------------------------------------------------------------- C ABI, no device
def test_gicp_symbol_and_workspace(lib):
    from buffer_amd import _lib
    assert "buf_gicp_batched" in _lib.exported_symbols()
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 4, 2) > 0
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 4, 2) == lib.buf_icp_ws_bytes(100_000, 100_000, 4, 1)   # the same record length
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 4, 3) == 0


def _call(lib, max_dist=0.1, epsilon=1e-3, src_normals=True, tgt_normals=True, src_len=(10, 20), tgt_len=(30, 40)):
    """buf_gicp_batched with placeholder device pointers: only argument checks may run (they precede any device call)."""
    fake, null = C.c_void_p(0x1000), C.c_void_p(0)
    sl, tl = np.array(src_len, np.int32), np.array(tgt_len, np.int32)
    rc = lib.buf_gicp_batched(fake, fake if src_normals else null, C.c_void_p(sl.ctypes.data), fake, fake if tgt_normals else null,
                              C.c_void_p(tl.ctypes.data), len(sl), max_dist, epsilon, fake, 30, 1e-6, 1e-6, fake, fake, fake, fake, null,
                              fake, 16, null)                             # (a workspace too small for anything: the last check of all)
    return rc, lib.buf_last_error().decode()


def test_gicp_batched_passes_its_argument_checks_up_to_the_workspace(lib):
    rc, msg = _call(lib)
    assert rc != 0 and "workspace" in msg


@pytest.mark.parametrize("max_dist", [0.0, -0.1, math.nan, math.inf])
def test_gicp_batched_rejects_a_bad_distance(lib, max_dist):
    rc, msg = _call(lib, max_dist=max_dist)
    assert rc == -1 and "max_dist" in msg and "buf_gicp_batched" in msg


@pytest.mark.parametrize("epsilon", [0.0, -1e-3, 1.0000001, math.nan, math.inf])
def test_gicp_batched_rejects_a_bad_epsilon(lib, epsilon):
    rc, msg = _call(lib, epsilon=epsilon)
    assert rc == -1 and "epsilon" in msg


def test_gicp_batched_rejects_negative_lengths_and_null_normals(lib):
    rc, msg = _call(lib, src_len=(10, -1))
    assert rc == -1 and "negative" in msg
    rc, msg = _call(lib, tgt_len=(-5, 40))
    assert rc == -1 and "negative" in msg
    rc, msg = _call(lib, src_normals=False)
    assert rc == -1 and "normals" in msg
    rc, msg = _call(lib, tgt_normals=False)
    assert rc == -1 and "normals" in msg


# ---------------------------------------------------------------------------------------------------- Python, no device
class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def test_generalized_python_checks_come_before_the_device_check():
    from buffer_amd import icp, ops
    assert ops.ICP_METHODS['generalized'] == 2
    s, t = [_Shape(5, 3)], [_Shape(7, 3)]
    with pytest.raises(ValueError, match="normals"):
        icp.icp_batched(s, t, 0.1, method='generalized')
    with pytest.raises(ValueError, match="normals"):
        icp.icp_batched(s, t, 0.1, method='generalized', tgt_normals=t)
    with pytest.raises(ValueError, match="src_normals"):
        icp.icp_batched(s, t, 0.1, method='generalized', src_normals=[_Shape(6, 3)], tgt_normals=t)
    with pytest.raises(ValueError, match="tgt_normals"):
        icp.icp_batched(s, t, 0.1, method='generalized', src_normals=s, tgt_normals=[])
    for eps in (0.0, -1.0, 1.5, math.nan):
        with pytest.raises(ValueError, match="epsilon"):
            icp.icp_batched(s, t, 0.1, method='generalized', src_normals=s, tgt_normals=t, epsilon=eps)
        with pytest.raises(ValueError, match="epsilon"):
            icp.icp_generalized(None, None, None, None, 0.1, epsilon=eps)
    with pytest.raises(RuntimeError, match="device"):                     # well-formed arguments reach the device check
        icp.icp_batched(s, t, 0.1, method='generalized', src_normals=s, tgt_normals=t)


def test_open3d_standin_has_generalized_icp():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    reg = o3d.pipelines.registration
    est = reg.TransformationEstimationForGeneralizedICP()
    assert est.epsilon == 1e-3 and est.kernel is None
    assert reg.TransformationEstimationForGeneralizedICP(epsilon=0.01).epsilon == 0.01
    with pytest.raises(NotImplementedError):
        reg.TransformationEstimationForGeneralizedICP(kernel=object())
    assert callable(reg.registration_generalized_icp)


# ---------------------------------------------------------------------------------------------------- driver plumbing, no device
def test_refine_options_on_all_three_drivers():
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert (a.refine, a.refine_dist, a.refine_iters) == (None, None, 30)
        a, _ = mod.parse_args(['--root', 'r', '--refine', 'generalized', '--refine-dist', '0.2', '--refine-iters', '7'])
        assert (a.refine, a.refine_dist, a.refine_iters) == ('generalized', 0.2, 7)
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--refine', 'colored'])


class _Pipe:
    """register_batches / refine_batch answer from the seeds alone and record the refine argument"""

    def __init__(self):
        import torch
        self.device, self.seen = torch.device('cpu'), []

    def refine_batch(self, inps, poses, **kw):
        import torch
        B = len(poses)
        return dict(poses=torch.stack([p * 2 for p in poses]) if B else torch.zeros((0, 4, 4)), fitness=torch.full((B,), 0.5, dtype=torch.float64),
                    inlier_rmse=torch.zeros(B, dtype=torch.float64), iterations=torch.full((B,), 3, dtype=torch.int32))

    def register_batches(self, batches, seeds=None, metrics_gt=None, **kw):
        import torch
        self.seen.append(kw)
        out = []
        for ch in seeds:
            res = [torch.eye(4) * (s + 1) for s in ch]
            if metrics_gt is not None:
                res = (res, torch.full((len(ch), 7), ch[0], dtype=torch.int32))
            out.append((res, self.refine_batch(None, res if metrics_gt is None else res[0])) if kw.get('refine') is not None else res)
        return out


class _Set:
    def meta(self, index, device=None):
        return {'relt_pose': np.eye(4) * index}


def test_register_pairs_hands_refine_through_and_keeps_the_unrefined_results():
    import torch
    from buffer_amd import driver
    pipe, ref = _Pipe(), dict(method='generalized', max_dist=0.1, max_iteration=5)
    plain = driver.register_pairs(pipe, _Set(), range(5), 2)
    assert pipe.seen == [{}]                                              # no refine: register_batches is called as before
    poses, refined = driver.register_pairs(pipe, _Set(), range(5), 2, refine=ref)
    assert pipe.seen[-1] == dict(refine=ref) and torch.equal(poses, plain)
    assert torch.equal(refined['poses'], plain * 2) and refined['iterations'].tolist() == [3] * 5 and refined['fitness'].shape == (5,)
    p2, counts, r2 = driver.register_pairs(pipe, _Set(), range(5), 2, stage_metrics=True, refine=ref)
    assert torch.equal(p2, plain) and counts.shape == (5, 7) and torch.equal(r2['poses'], refined['poses'])
    p0, r0 = driver.register_pairs(pipe, _Set(), [], 2, refine=ref)
    assert p0.shape == (0, 4, 4) and r0['poses'].shape == (0, 4, 4) and r0['iterations'].shape == (0,)
