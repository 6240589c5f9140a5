"""Pose-graph optimisation without a GPU: the float64 restatement (tests/posegraph_ref.py, written from the contract comment of
buf_pose_graph_optimize) against finite differences and planted scenes, the condition on the inputs of the GPU tests (every decision
of every scene keeps a margin), the host functions of buffer_amd/posegraph.py, and the argument errors of both layers, which are
raised before any device use (this file runs where there is no device)."""
import ctypes as C
import os

import numpy as np
import pytest

import posegraph_ref as R

EPS = np.finfo(np.float64).eps


def test_log_exp_round_trip_over_the_whole_range():
    """Log(Exp(a)) against a at the angles of the issue.  Bound: 4 eps |a| (relative, so the tiny angles are held to their own
    size): the quaternion, its norm, atan2 and the scaling round once each.  Measured here: <= 1.4 eps |a|."""
    rng = np.random.default_rng(0)
    for angle in (1e-12, 1e-9, 1e-4, 1.0, 3.0, np.pi - 1e-3, np.pi - 1e-9):
        worst = 0.0
        for _ in range(50):
            a = R.random_rotvec(rng, angle)
            worst = max(worst, float(np.abs(R.so3_log(R.so3_exp(a)) - a).max()))
        print(f'angle {angle:g}: max |Log(Exp(a)) - a| = {worst:.3g} = {worst / (EPS * angle):.2f} eps |a|')
        assert worst <= 4 * EPS * angle


def test_log_of_exactly_pi_and_of_the_identity():
    assert np.array_equal(R.so3_log(np.eye(3)), np.zeros(3))
    for axis in np.eye(3):
        phi = R.so3_log(2.0 * np.outer(axis, axis) - np.eye(3))
        assert abs(np.linalg.norm(phi) - np.pi) <= 4 * EPS * np.pi and abs(abs(phi @ axis) - np.pi) <= 4 * EPS * np.pi


@pytest.mark.parametrize("phi,bound", [(0.1, 2e-7), (0.01, 1e-9)])
def test_jacobians_against_central_differences(phi, bound):
    """The series of Jri is cut after P^2 / 12: the next term, |phi|^4 / 720, is what the Jacobian leaves (1.4e-7 at 0.1, 1.4e-11 at
    0.01, where the central difference's own eps / h = 2e-10 dominates).  Measured: 1.3e-7 and 1.6e-10."""
    rng = np.random.default_rng(1)
    Xi, Xj = R.random_motion(rng, 1.0, 1.0), R.random_motion(rng, 1.0, 1.0)
    Z = R.inv(Xi) @ Xj @ R.inv(R.random_motion(rng, phi, 0.2))
    r, Ji, Jj = R.jacobians(Xi, Xj, Z)
    assert abs(np.linalg.norm(r[:3]) - phi) < 1e-12
    h = 1e-6
    for which, J in ((0, Ji), (1, Jj)):
        num = np.zeros((6, 6))
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            f = lambda s: R.residual(R.retract(Xi, s * d[:3], s * d[3:]) if which == 0 else Xi,       # noqa: E731
                                     R.retract(Xj, s * d[:3], s * d[3:]) if which == 1 else Xj, Z)[0]
            num[:, c] = (f(1.0) - f(-1.0)) / (2 * h)
        err = float(np.abs(num - J).max())
        print(f'|phi| = {phi}: J_{"ij"[which]} differs from central differences by {err:.3g}')
        assert err <= bound


def test_zero_residual_graph_is_recovered():
    """exact measurements, free nodes 0.05 rad / m off: quadratic convergence, stopped by the step; the error is bounded by the
    step at which the solver stops (eps_step = 1e-9).  Measured: 4 solves, 9.9e-12."""
    g, W = R.scenes()['zero_residual']
    res = R.reference('zero_residual')
    print(res['status'], res['solves'], np.abs(res['poses'] - W).max())
    assert res['status'] == 'CONVERGED_STEP' and res['solves'] <= 5
    assert np.abs(res['poses'] - W).max() <= 1e-9 and res['cost_final'] <= 1e-15 * res['cost_initial']


def test_outlier_scene_line_process_switches_off_exactly_the_false_edges():
    """n = 12, 4 false chords (0.6 rad / 0.7 m), all edges uncertain, chain init.  The figures of the issue as bounds: false edges
    end at l <= 1.3e-5, true ones at l >= 0.96, pruning at 0.25 removes exactly the false ones, at most 5 solves, the worst fragment
    within 9 mm of its planted pose; without the line process (mu = 0) it is decimetres off (measured here: l 1.15e-5 / 0.988,
    4 solves, 2.8 mm against 0.27 m)."""
    from buffer_amd import posegraph
    g, W, false = R.make_scene(0)
    res = R.reference('outlier')
    err = posegraph.trajectory_error(res['poses'], W)
    off = posegraph.trajectory_error(R.optimize(dict(g, mu=0.0))['poses'], W)
    print(res['status'], res['solves'], res['weights'][false].max(), res['weights'][~false].min(), err['rte'].max(), off['rte'].max())
    assert res['weights'][false].max() <= 1.3e-5 and res['weights'][~false].min() >= 0.96
    assert np.array_equal(posegraph.prune(res, 0.25), false)
    assert res['status'].startswith('CONVERGED') and res['solves'] <= 5
    assert err['rte'].max() <= 0.009 and off['rte'].max() >= 0.2 and off['rte'].max() >= 25 * err['rte'].max()


def test_gpu_scenes_keep_their_margins():
    """A condition on the INPUTS of the GPU tests: at every solve of the restatement's trace max |delta| is at least 10 x away from
    eps_step, an accepted step's cost ratio at least 10 x away from eps_cost, and |rho| >= 0.01 (the device and the restatement
    differ in rho by rounding, ~1e-12: a rho of 0.01 is far more than 10 x away from changing its sign).  With these margins equal
    status / solves / accepted counts are a fair demand.  A seed that fails is replaced in posegraph_ref.scenes()."""
    for name in R.scenes():
        for iters in (100, 1):
            m = R.margins(R.reference(name, iters)['trace'])
            print(name, iters, m)
            assert m['rho'] >= 0.01 and m['step'] >= 10 and m['cost'] >= 10, (name, iters, m)
    tr = R.reference('rejected')['trace']
    rejected = [t for t in tr if t['factored'] and not t['accepted'] and np.isfinite(t['rho'])]
    assert len(rejected) >= 1 and all(t['rho'] < 0 for t in rejected), 'the rejected-solve scene has no rejected solve'
    neg = R.optimize(R.negative_definite_scene())
    assert (neg['status'], neg['solves'], neg['accepted']) == ('STALLED', 14, 0)


# ---------------------------------------------------------------------------------------------------- host functions
def _edge(i, j, T=None, count=100.0):
    info = np.eye(6)
    info[3:, 3:] *= count
    return dict(i=i, j=j, T=np.eye(4) if T is None else T, info=info, uncertain=True)


def test_initial_poses_spanning_tree_ties_and_disconnected_nodes():
    from buffer_amd import posegraph
    rng = np.random.default_rng(2)
    W = R.chain_world(rng, 6)
    rel = lambda i, j: R.inv(W[i]) @ W[j]                                              # noqa: E731
    wrong = R.random_motion(rng, 0.5, 0.5)
    edges = [_edge(0, 1, rel(0, 1), 50), _edge(1, 2, rel(1, 2) @ wrong, 10), _edge(0, 2, rel(0, 2), 80),      # 1-2 loses to 0-2
             _edge(3, 2, rel(3, 2), 80),                                                                       # given as (j, i)
             _edge(2, 3, rel(2, 3) @ wrong, 80)]                                                               # a tie: the lower index wins
    X, lost = posegraph.initial_poses(6, edges, fixed=0)
    assert lost == [4, 5] and np.array_equal(X[4], np.eye(4)) and np.array_equal(X[5], np.eye(4))
    np.testing.assert_allclose(X[:4], W[:4], atol=1e-14)
    X2, lost2 = posegraph.initial_poses(6, edges, fixed=3)                               # another root: the same tree, re-based
    assert lost2 == [4, 5]
    np.testing.assert_allclose(np.array([R.inv(X2[0]) @ x for x in X2[:4]]), W[:4], atol=1e-14)
    assert posegraph.initial_poses(0, [])[0].shape == (0, 4, 4)
    with pytest.raises(ValueError):
        posegraph.initial_poses(3, [], fixed=3)


def test_info_from_3dmatch_inverts_information_matrix():
    from buffer_amd import pairs, posegraph
    rng = np.random.default_rng(3)
    u = rng.uniform(-1, 1, (200, 3))
    sum_uu = [(u[:, a] * u[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    a3 = pairs.information_matrix(200, u.sum(0), sum_uu, '3dmatch')
    o3 = pairs.information_matrix(200, u.sum(0), sum_uu, 'open3d')
    np.testing.assert_allclose(posegraph.info_from_3dmatch(a3), o3, rtol=0, atol=1e-12)
    np.testing.assert_allclose(o3, R.points_info(rng, 0) + sum(np.hstack([-R.hat(p), np.eye(3)]).T @ np.hstack([-R.hat(p), np.eye(3)]) for p in u),
                               rtol=0, atol=1e-10)
    mu = posegraph.line_process_weight([dict(info=o3, uncertain=True), dict(info=7 * o3, uncertain=False)], 0.05, 2.0)
    assert mu == pytest.approx(2.0 * 0.05 ** 2 * 200) and posegraph.line_process_weight([dict(info=o3)], 0.05) == 0.0


def test_trajectory_write_then_read_poses(tmp_path):
    from buffer_amd import pairs, posegraph
    W = R.chain_world(np.random.default_rng(4), 5)
    path = str(tmp_path / 'scene' / 'traj.log')
    posegraph.write_trajectory(path, W)
    back = pairs.read_poses(path, 5, None)
    assert np.array_equal(np.array(back), W)                       # repr(float) round-trips


def test_trajectory_error_under_a_common_rigid_motion():
    from buffer_amd import posegraph
    rng = np.random.default_rng(5)
    W = R.chain_world(rng, 6)
    move = R.random_motion(rng, 1.0, 3.0)
    moved = np.array([move @ w for w in W])
    e = posegraph.trajectory_error(moved, W, fixed=2)
    assert e['rte'].max() <= 1e-13 and e['rre'].max() <= 1e-10 and e['rte_rmse'] <= 1e-13
    bent = moved.copy()
    bent[4] = bent[4] @ R.pose(R.so3_exp([0.0, 0.0, np.radians(3.0)]), [0.0, 0.04, 0.03])
    e = posegraph.trajectory_error(bent, W, fixed=2)
    assert e['rre'][4] == pytest.approx(3.0, abs=1e-9) and np.delete(e['rre'], 4).max() <= 1e-10
    assert e['rte'][4] == pytest.approx(np.linalg.norm(W[2][:3, :3].T @ W[4][:3, :3] @ np.array([0.0, 0.04, 0.03])), abs=1e-12)


def test_project_rigid_and_prune():
    from buffer_amd import posegraph
    T = R.random_motion(np.random.default_rng(6), 0.8, 1.0)
    noisy = T.astype(np.float32).astype(np.float64)
    noisy[:3, :3] += 1e-4
    P = posegraph.project_rigid(noisy)
    assert np.abs(P[:3, :3].T @ P[:3, :3] - np.eye(3)).max() <= 4 * EPS and np.linalg.det(P[:3, :3]) > 0
    assert np.abs(P - T).max() <= 3e-4 and np.array_equal(P[3], [0, 0, 0, 1])
    assert np.array_equal(posegraph.prune(dict(weights=[1.0, 0.2, 0.25, 1e-6]), 0.25), [False, True, False, True])
    assert np.array_equal(posegraph.prune(dict(weights=[0.1, 0.1]), 0.25, uncertain=[True, False]), [True, False])


def test_optimize_rejects_bad_arguments_before_any_device_use():
    """No device is needed (or present, where this file runs): every check comes before the first use of torch."""
    from buffer_amd import posegraph
    good = dict(n=3, edges=[_edge(0, 1), _edge(1, 2)], init=np.tile(np.eye(4), (3, 1, 1)), fixed=0, mu=1.0)
    bad = [dict(good, n=-1), dict(good, fixed=3), dict(good, fixed=-1), dict(good, mu=-1.0), dict(good, mu=float('nan')),
           dict(good, edges=[_edge(0, 3)]), dict(good, edges=[_edge(-1, 1)]), dict(good, edges=[_edge(1, 1)]),
           dict(good, init=np.tile(np.eye(4), (2, 1, 1))), dict(good, n=129, init=np.tile(np.eye(4), (129, 1, 1)))]
    for g in bad:
        with pytest.raises(ValueError):
            posegraph.optimize([good, g])
    for kw in (dict(max_iterations=-1), dict(eps_step=0.0), dict(eps_cost=float('nan')), dict(tau0=float('inf')), dict(tau0=-1.0)):
        with pytest.raises(ValueError):
            posegraph.optimize([good], **kw)
    assert posegraph.optimize([]) == []


def _abi_call(L, kw, null=()):
    """buf_pose_graph_optimize with host values and device pointers that are never dereferenced on the host (address 16)"""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)                                  # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)                                            # noqa: E731
    one = C.c_void_p(16)
    nd, ed, ei, ej, fx = i32(kw['nodes']), i32(kw['edges']), i32(kw['edge_i']), i32(kw['edge_j']), i32(kw['fixed'])
    un, mu = np.ascontiguousarray(kw['uncertain'], np.uint8), np.ascontiguousarray(kw['mu'], np.float64)
    p = dict(Z=one, info=one, X0=one, X=one, status=one, cost=one, edge=one, ws=one)
    p.update({k: None for k in null})
    return L.buf_pose_graph_optimize(hp(nd), hp(ed), kw.get('ngraphs', len(nd)), hp(ei), hp(ej), p['Z'], p['info'], hp(un), hp(fx), hp(mu),
                                     p['X0'], kw['max_iterations'], kw['eps_step'], kw['eps_cost'], kw['tau0'], p['X'], p['status'],
                                     p['cost'], p['edge'], p['ws'], C.c_size_t(kw.get('ws_bytes', 1 << 30)), None)


def test_c_abi_argument_errors_come_before_any_device_work():
    """Every BUF_EINVAL case of the header, BUF_ECAPACITY and BUF_EWORKSPACE, on a machine without a device: the device pointers
    are the address 16, so a call that went past its checks would not return an error code."""
    from buffer_amd import _lib, build
    build.build()
    L = _lib.lib()
    base = R.abi_base()
    for name, change in R.einval_cases().items():
        assert _abi_call(L, dict(base, **change)) == -1, name
        assert b'buf_pose_graph_optimize' in L.buf_last_error(), name
    assert _abi_call(L, dict(base, ngraphs=-1)) == -1
    for null in ('Z', 'info', 'X0', 'X', 'status', 'cost', 'edge', 'ws'):
        assert _abi_call(L, base, null=(null,)) == -1, null
    assert _abi_call(L, dict(base, ngraphs=0)) == 0                                                 # nothing to do, nothing touched
    big = dict(base, nodes=[129], edges=[1], edge_i=[0], edge_j=[128], uncertain=[0])
    assert _abi_call(L, big) == -4 and b'capacity' in L.buf_last_error()                            # BUF_ECAPACITY
    assert _abi_call(L, dict(base, ws_bytes=16)) == -3                                              # BUF_EWORKSPACE
    ws = L.buf_pose_graph_ws_bytes
    assert ws(1, 128, 1000, 128) > 2 * 8 * 762 * 762 and ws(0, 0, 0, 0) == 0 and ws(1, 129, 1, 129) == 0 and ws(1, -1, 0, 1) == 0
    assert ws(2, 6, 4, 3) < ws(2, 6, 4, 4) and os.path.exists(_lib.LIB_PATH)
