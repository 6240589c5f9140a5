"""buf_pose_graph_optimize (csrc/posegraph.hip) on the device against the float64 restatement tests/posegraph_ref.py, scene by
scene of posegraph_ref.scenes(): the costs and weights at the initial poses, one step, the full loop (status, solves and accepted
counts EQUAL: test_posegraph_cpu.py holds every decision of these scenes at a 10 x margin), sizes whose 6 (n - 1) unknowns hit the
block edges of the factorisation, batch composition bit for bit, and the failure statuses.

Kernel and restatement are both fp64; they differ in the order of their sums, in the Cholesky (blocked, right-looking, against
LAPACK) and in sin / cos / atan2 / sqrt by an ulp.  Every tolerance of TOL is at most 2 x the measurement printed beside it and none
exceeds eps_step = 1e-9: a disagreement larger than the step at which the solver itself stops would be a different answer.
Poses and weights compare absolutely; costs and q_e with used = |d| / (tol (1 + |want|))."""
import numpy as np
import pytest
import torch

import posegraph_ref as R
from util import assert_close

# key: (tolerance, measured on an MI355X).  Keys: <test>/<scene>/<quantity>.
TOL = {
    'zero/outlier/poses': (0.0e+00, 0.000e+00),
    'zero/outlier/costs': (3.7e-16, 1.863e-16),
    'zero/outlier/weights': (6.4e-15, 3.220e-15),
    'zero/outlier/q': (2.9e-15, 1.485e-15),
    'zero/rejected/poses': (0.0e+00, 0.000e+00),
    'zero/rejected/costs': (0.0e+00, 0.000e+00),
    'zero/rejected/weights': (0.0e+00, 0.000e+00),
    'zero/rejected/q': (8.7e-16, 4.387e-16),
    'zero/n128/poses': (0.0e+00, 0.000e+00),
    'zero/n128/costs': (6.7e-16, 3.373e-16),
    'zero/n128/weights': (0.0e+00, 0.000e+00),
    'zero/n128/q': (2.7e-14, 1.395e-14),
    'step/outlier/poses': (4.4e-16, 2.220e-16),
    'step/outlier/costs': (3.7e-16, 1.863e-16),
    'step/outlier/weights': (2.2e-15, 1.110e-15),
    'step/outlier/q': (1.0e-15, 5.006e-16),
    'step/rejected/poses': (0.0e+00, 0.000e+00),
    'step/rejected/costs': (0.0e+00, 0.000e+00),
    'step/rejected/weights': (0.0e+00, 0.000e+00),
    'step/rejected/q': (8.7e-16, 4.387e-16),
    'step/zero_residual/poses': (3.3e-16, 1.665e-16),
    'step/zero_residual/costs': (7.7e-16, 3.898e-16),
    'step/zero_residual/weights': (0.0e+00, 0.000e+00),
    'step/zero_residual/q': (5.9e-16, 2.997e-16),
    'step/n44/poses': (7.1e-15, 3.553e-15),
    'step/n44/costs': (9.2e-15, 4.613e-15),
    'step/n44/weights': (0.0e+00, 0.000e+00),
    'step/n44/q': (3.6e-15, 1.836e-15),
    'step/n128/poses': (2.5e-14, 1.288e-14),
    'step/n128/costs': (4.6e-15, 2.335e-15),
    'step/n128/weights': (0.0e+00, 0.000e+00),
    'step/n128/q': (1.8e-14, 9.272e-15),
    'full/isolated/poses': (6.6e-16, 3.331e-16),
    'full/isolated/costs': (2.3e-15, 1.168e-15),
    'full/isolated/weights': (0.0e+00, 0.000e+00),
    'full/isolated/q': (1.2e-15, 6.197e-16),
    'full/n128/poses': (2.2e-15, 1.110e-15),
    'full/n128/costs': (1.5e-14, 7.885e-15),
    'full/n128/weights': (0.0e+00, 0.000e+00),
    'full/n128/q': (7.7e-15, 3.885e-15),
    'full/n2/poses': (2.2e-16, 1.110e-16),
    'full/n2/costs': (5.3e-16, 2.685e-16),
    'full/n2/weights': (0.0e+00, 0.000e+00),
    'full/n2/q': (2.6e-26, 1.317e-26),
    'full/n23/poses': (1.1e-15, 5.551e-16),
    'full/n23/costs': (2.3e-15, 1.154e-15),
    'full/n23/weights': (0.0e+00, 0.000e+00),
    'full/n23/q': (1.2e-15, 6.300e-16),
    'full/n3/poses': (4.4e-16, 2.220e-16),
    'full/n3/costs': (1.3e-15, 6.871e-16),
    'full/n3/weights': (0.0e+00, 0.000e+00),
    'full/n3/q': (2.2e-16, 1.146e-16),
    'full/n44/poses': (1.3e-15, 6.661e-16),
    'full/n44/costs': (2.4e-15, 1.236e-15),
    'full/n44/weights': (0.0e+00, 0.000e+00),
    'full/n44/q': (2.4e-15, 1.249e-15),
    'full/outlier/poses': (4.4e-16, 2.220e-16),
    'full/outlier/costs': (3.7e-16, 1.863e-16),
    'full/outlier/weights': (2.6e-15, 1.332e-15),
    'full/outlier/q': (1.7e-15, 8.710e-16),
    'full/outlier_fixed11/poses': (4.4e-16, 2.220e-16),
    'full/outlier_fixed11/costs': (1.4e-15, 7.454e-16),
    'full/outlier_fixed11/weights': (3.9e-15, 1.998e-15),
    'full/outlier_fixed11/q': (1.6e-15, 8.461e-16),
    'full/outlier_fixed5/poses': (6.6e-16, 3.331e-16),
    'full/outlier_fixed5/costs': (7.4e-16, 3.727e-16),
    'full/outlier_fixed5/weights': (2.2e-15, 1.110e-15),
    'full/outlier_fixed5/q': (1.0e-15, 5.037e-16),
    'full/rejected/poses': (1.1e-15, 5.551e-16),
    'full/rejected/costs': (2.0e-15, 1.028e-15),
    'full/rejected/weights': (0.0e+00, 0.000e+00),
    'full/rejected/q': (9.6e-16, 4.813e-16),
    'full/rot179/poses': (4.4e-16, 2.220e-16),
    'full/rot179/costs': (3.9e-16, 1.991e-16),
    'full/rot179/weights': (2.6e-15, 1.332e-15),
    'full/rot179/q': (2.1e-15, 1.089e-15),
    'full/swap_duplicates/poses': (4.9e-16, 2.498e-16),
    'full/swap_duplicates/costs': (7.3e-16, 3.698e-16),
    'full/swap_duplicates/weights': (3.1e-15, 1.554e-15),
    'full/swap_duplicates/q': (1.8e-15, 9.244e-16),
    'full/zero_residual/poses': (2.2e-16, 1.110e-16),
    'full/zero_residual/costs': (3.2e-16, 1.632e-16),
    'full/zero_residual/weights': (0.0e+00, 0.000e+00),
    'full/zero_residual/q': (3.5e-25, 1.755e-25),
    'stall/negdef/costs': (1.3e-16, 6.611e-17),
}
assert all(t <= 1e-9 and t <= 2.0 * m for t, m in TOL.values())


def _check(key, got, want, mixed=False):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    d = np.abs(got - want) / ((1.0 + np.abs(want)) if mixed else 1.0)
    print(f'MEAS {key} {float(d.max()) if d.size else 0.0:.3e}')
    tol = TOL[key][0]
    if tol == 0.0:
        assert np.array_equal(got, want), key
    else:
        assert_close(got, want, rtol=tol if mixed else 0.0, atol=tol, name=key)


def _run(graphs, **kw):
    from buffer_amd import posegraph
    return posegraph.optimize(graphs, **kw)


def _compare(test, name, got, want):
    assert (got['status'], got['solves'], got['accepted']) == (want['status'], want['solves'], want['accepted']), name
    _check(f'{test}/{name}/poses', got['poses'], want['poses'])
    _check(f'{test}/{name}/costs', [got['cost_initial'], got['cost_final']], [want['cost_initial'], want['cost_final']], mixed=True)
    _check(f'{test}/{name}/weights', got['weights'], want['weights'])
    _check(f'{test}/{name}/q', got['residuals'], want['residuals'], mixed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ['outlier', 'rejected', 'n128'])
def test_zero_iterations_give_the_costs_and_weights_at_the_initial_poses(dev, name):
    g = R.scenes()[name][0]
    got, want = _run([g], max_iterations=0)[0], R.reference(name, 0)
    assert want['status'] == 'MAX_ITER' and want['solves'] == 0
    _compare('zero', name, got, want)
    assert np.array_equal(got['poses'], g['init']) and got['cost_initial'] == got['cost_final']


@pytest.mark.gpu
@pytest.mark.parametrize("name", ['outlier', 'rejected', 'zero_residual', 'n44', 'n128'])
def test_one_step(dev, name):
    g = R.scenes()[name][0]
    got, want = _run([g], max_iterations=1)[0], R.reference(name, 1)
    assert want['solves'] == 1
    _compare('step', name, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.scenes()))
def test_full_loop(dev, name):
    """the outlier scene (fixed node 0, a middle node, the last node), the rejected-solve scene, the zero-residual scene, n = 2, 3,
    23, 44, 128 (6 (n - 1) = 6, 12, 132, 258, 762: one block, a tail of 4, tails next to multiples of 8 and of the 256 threads, the
    capacity), duplicate and (j, i) edges, an isolated node, a false edge 179.9 degrees off"""
    g, W = R.scenes()[name]
    got, want = _run([g])[0], R.reference(name)
    _compare('full', name, got, want)
    assert np.array_equal(got['poses'][g['fixed']], g['init'][g['fixed']])
    if name == 'isolated':
        assert np.array_equal(got['poses'][-1], g['init'][-1])
    if name == 'rejected':
        assert got['solves'] - got['accepted'] == 3
    if name == 'rot179':                                             # the edge that lives next to pi is the one switched off hardest
        k = int(np.argmin(want['weights']))
        assert got['weights'][k] < 1e-6 and np.argmin(got['weights']) == k and np.isfinite(got['residuals']).all()
    if name.startswith('outlier'):
        from buffer_amd import posegraph
        false = R.make_scene(0, fixed=g['fixed'])[2]
        assert np.array_equal(posegraph.prune(got), false)
        assert posegraph.trajectory_error(got['poses'], W, g['fixed'])['rte'].max() < 0.009


@pytest.mark.gpu
def test_two_pass_prunes_the_false_edges_and_keeps_the_rest(dev):
    from buffer_amd import posegraph
    g, W, false = R.make_scene(0)
    res = posegraph.optimize_two_pass([g, R.scenes()['n3'][0]])
    assert np.array_equal(res[0]['pruned'], false) and not res[1]['pruned'].any()
    assert len(res[0]['weights']) == int((~false).sum()) and res[0]['weights'].min() > 0.96
    assert res[0]['status'].startswith('CONVERGED') and posegraph.trajectory_error(res[0]['poses'], W)['rte'].max() < 0.009
    assert np.array_equal(res[1]['first']['poses'], _run([R.scenes()['n3'][0]])[0]['poses'])


@pytest.mark.gpu
def test_capacity_and_nothing_to_do(dev):
    from buffer_amd import _lib, ops, posegraph
    eye = lambda n: np.tile(np.eye(4), (n, 1, 1))                                      # noqa: E731
    with pytest.raises(ValueError, match='capacity'):
        posegraph.optimize([dict(n=129, edges=[], init=eye(129), fixed=0, mu=0.0)])
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dev)                   # noqa: E731
    with pytest.raises(_lib.BufferHipError, match=r'\(-4\)'):                          # BUF_ECAPACITY from the library itself
        ops.pose_graph_optimize([129], [1], [0], [128], t(eye(1)), t(np.eye(6)[None]), [0], [0], [0.0], t(eye(129)))
    lone = R.random_motion(np.random.default_rng(1), 0.5, 0.5)
    e = dict(i=0, j=1, T=lone, info=R.points_info(np.random.default_rng(2), 300), uncertain=False)
    res = _run([dict(n=1, edges=[], init=lone[None], fixed=0, mu=0.0),                 # N = 1
                dict(n=3, edges=[], init=np.array([lone, np.eye(4), lone]), fixed=1, mu=1.0),      # E = 0
                dict(n=0, edges=[], init=np.zeros((0, 4, 4)), fixed=0, mu=0.0),
                dict(n=2, edges=[dict(e, info=-e['info'])], init=eye(2), fixed=0, mu=0.0)])        # max diag H < 0: lambda0 not > 0
    for r, n in zip(res, (1, 3, 0, 2)):
        assert (r['status'], r['solves'], r['accepted']) == ('NOTHING', 0, 0) and r['poses'].shape == (n, 4, 4)
    assert np.array_equal(res[0]['poses'][0], lone) and np.array_equal(res[1]['poses'][2], lone)
    assert res[0]['cost_initial'] == 0.0 and res[1]['cost_final'] == 0.0 and res[3]['cost_initial'] == res[3]['cost_final'] < 0.0
    assert np.array_equal(res[3]['poses'], eye(2))
    X, status, cost, edge = ops.pose_graph_optimize([], [], [], [], t(np.zeros((0, 4, 4))), t(np.zeros((0, 6, 6))), [], [], [], t(np.zeros((0, 4, 4))))
    assert X.shape == (0, 4, 4) and status.shape == (0, 3)


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ('poses', 'weights', 'residuals')) and \
        all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in ('status', 'solves', 'accepted', 'cost_initial', 'cost_final'))


@pytest.mark.gpu
def test_batch_of_six_keeps_every_graphs_bits(dev):
    """six graphs of different sizes: called twice, reversed, each alone; then one of them with a NaN in Z returns FAILED with its
    initial poses while its neighbours keep their bits"""
    names = ['n2', 'outlier', 'n44', 'rejected', 'n3', 'swap_duplicates']
    graphs = [R.scenes()[k][0] for k in names]
    first = _run(graphs)
    again = _run(graphs)
    rev = _run(graphs[::-1])[::-1]
    for k, name in enumerate(names):
        alone = _run([graphs[k]])[0]
        assert _same(first[k], again[k]) and _same(first[k], rev[k]) and _same(first[k], alone), name
        want = R.reference(name)
        assert (first[k]['status'], first[k]['solves'], first[k]['accepted']) == (want['status'], want['solves'], want['accepted'])
    bad = dict(graphs[2], edges=[dict(e) for e in graphs[2]['edges']])
    bad['edges'][5]['T'] = bad['edges'][5]['T'].copy()
    bad['edges'][5]['T'][1, 3] = np.nan
    mixed = _run(graphs[:2] + [bad] + graphs[3:])
    assert mixed[2]['status'] == 'FAILED' and mixed[2]['solves'] == 0 and np.array_equal(mixed[2]['poses'], bad['init'])
    assert np.isnan(mixed[2]['cost_initial']) and np.isnan(mixed[2]['weights']).all()
    assert _same(mixed[2], {k: v for k, v in R.optimize(bad).items()})
    for k in (0, 1, 3, 4, 5):
        assert _same(first[k], mixed[k]), names[k]
    for what, val in (('init', np.inf), ('info', -np.inf)):
        bad = dict(graphs[1], edges=[dict(e) for e in graphs[1]['edges']], init=graphs[1]['init'].copy())
        if what == 'init':
            bad['init'][3, 0, 0] = val
        else:
            bad['edges'][0]['info'] = bad['edges'][0]['info'].copy()
            bad['edges'][0]['info'][2, 2] = val
        r = _run([graphs[0], bad])
        assert r[1]['status'] == 'FAILED' and np.array_equal(r[1]['poses'], bad['init']) and _same(r[0], first[0]), what


@pytest.mark.gpu
def test_negative_definite_information_stalls_at_the_initial_poses(dev):
    """posegraph_ref.negative_definite_scene: lambda0 > 0 but no lambda below 1e30 lambda0 makes H + lambda I positive definite; every
    factorisation fails at a pivot, 14 rejected solves, STALLED, the poses are the initial ones bit for bit"""
    g = R.negative_definite_scene()
    got, want = _run([g])[0], R.optimize(g)
    assert (got['status'], got['solves'], got['accepted']) == (want['status'], want['solves'], want['accepted']) == ('STALLED', 14, 0)
    assert np.array_equal(got['poses'], g['init']) and got['cost_initial'] == got['cost_final']
    _check('stall/negdef/costs', [got['cost_initial']], [want['cost_initial']], mixed=True)


@pytest.mark.gpu
def test_every_einval_case_of_the_header(dev):
    from buffer_amd import _lib, ops
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dev)                   # noqa: E731
    eye = np.tile(np.eye(4), (3, 1, 1))

    def call(nodes, edges, edge_i, edge_j, uncertain, fixed, mu, **kw):
        return ops.pose_graph_optimize(nodes, edges, edge_i, edge_j, t(eye[:2]), t(np.tile(np.eye(6), (2, 1, 1))), uncertain, fixed, mu, t(eye), **kw)
    base = R.abi_base()
    status = call(**base)[1].cpu().numpy()
    assert status[0, 0] in (1, 2)                                   # the base call is a valid one: converged at zero residuals
    for name, change in R.einval_cases().items():
        kw = dict(base, **change)
        if name in ('negative_nodes', 'negative_edges'):            # (the wrapper's own check: the counts size its outputs)
            with pytest.raises(ValueError):
                call(**kw)
            continue
        with pytest.raises(_lib.BufferHipError, match=r'\(-1\)'):
            call(**kw)
