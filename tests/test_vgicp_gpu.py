"""Voxelized Generalized ICP on the device (csrc/vgicp.hip: buf_voxel_map_build, buf_vgicp_batched, icp.voxel_map / icp.vgicp_batched)
against the float64 restatement tests/vgicp_ref.py.  The voxel map is compared exactly (kernel and restatement run the same fp64
operations in the same order); rows, term counts, fitness and update counts are compared exactly under the margin conditions
tests/test_vgicp_cpu.py asserts; T and rmse differ in the order of their sums, the 3x3 inverse (cofactors against LU) and the 6x6 solve
(LDL^T against LU) and are held at 2 x the printed measurement (tests/util.assert_close)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gicp_ref
import vgicp_ref
from util import assert_close

pytestmark = pytest.mark.gpu

V, EPS = vgicp_ref.VOXEL, vgicp_ref.EPSILON


def _dev(a, dev):
    return torch.from_numpy(np.array(a, np.float32).reshape(-1, 3)).to(dev)


def _same(a, b):
    return (np.array_equal(a['T'], b['T']) and a['fitness'] == b['fitness'] and a['inlier_rmse'] == b['inlier_rmse']
            and a['iterations'] == b['iterations'] and ('rows' not in a or np.array_equal(a['rows'], b['rows'])))


@pytest.fixture(scope="module", autouse=True)
def before_voxelized(dev):
    """point-to-point, point-to-plane and generalized results of two pairs, taken before this module makes its first voxelized call:
    test_the_other_methods_keep_their_bits repeats the calls afterwards"""
    from buffer_amd import icp
    sc = gicp_ref.scene()
    S, SN = [_dev(sc['src'], dev), _dev(sc['src'][:257], dev)], [_dev(sc['src_normals'], dev), _dev(sc['src_normals'][:257], dev)]
    Tg, N = [_dev(sc['tgt'], dev), _dev(sc['tgt'][:1500], dev)], [_dev(sc['tgt_normals'], dev), _dev(sc['tgt_normals'][:1500], dev)]
    call = dict(p2p=lambda: icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, max_iteration=40),
                p2l=lambda: icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, method='point_to_plane', tgt_normals=N, max_iteration=40),
                gicp=lambda: icp.icp_batched(S, Tg, gicp_ref.MAX_DIST, method='generalized', src_normals=SN, tgt_normals=N, max_iteration=40))
    return call, {k: f() for k, f in call.items()}


@pytest.fixture(scope="module")
def scene_map(dev):
    """the scene's target map at voxel 0.2, on the device and restated; shared, never written"""
    from buffer_amd import icp
    sc = vgicp_ref.scene()
    return icp.voxel_map([_dev(sc['tgt'], dev)], V, [_dev(sc['tgt_normals'], dev)], EPS), vgicp_ref.build_map(sc['tgt'], sc['tgt_normals'], V, EPS)


def _scene_run(dev, vmap, nb, **kw):
    from buffer_amd import icp
    sc = vgicp_ref.scene()
    return icp.vgicp_batched([_dev(sc['src'], dev)], vmap, src_normals=[_dev(sc['src_normals'], dev)], neighbors=nb, return_rows=True, **kw)[0]


# ---------------------------------------------------------------------------------------------------- the map
def _rows(vmap):
    return {k: v.cpu().numpy() for k, v in vmap.rows().items()}


def _check_map(dev, clouds, normals, voxel, eps=EPS):
    """one device map of all clouds == the restatement of each cloud, every array exactly"""
    from buffer_amd import icp
    vm = icp.voxel_map([_dev(c, dev) for c in clouds], voxel, None if normals is None else [_dev(n, dev) for n in normals], eps)
    got = _rows(vm)
    assert vm.nclouds == len(clouds) and vm.voxel == voxel and vm.epsilon == eps and got['row_off'][0] == 0
    for c, cloud in enumerate(clouds):
        want = vgicp_ref.build_map(cloud, None if normals is None else normals[c], voxel, eps)
        lo, hi = got['row_off'][c], got['row_off'][c + 1]
        assert hi - lo == len(want['keys']), c
        for k in ('keys', 'counts', 'means', 'covs'):
            assert np.array_equal(got[k][lo:hi], want[k]), (c, k)
    assert got['row_off'][-1] == vm.nrows == len(got['keys'])
    return vm, got


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("voxel", [0.2, 0.05])
def test_map_of_the_scene_target_is_the_restatement(dev, voxel):
    sc = vgicp_ref.scene()
    vm, got = _check_map(dev, [sc['tgt']], [sc['tgt_normals']], voxel)
    assert got['counts'].sum() == 1800 and (np.diff(got['keys']) > 0).all()
    print(f'voxel {voxel}: {vm.nrows} rows, largest count {got["counts"].max()}')


def test_hand_computed_map(dev):
    pts = vgicp_ref.HAND_POINTS
    nrm = np.zeros_like(pts)
    nrm[:, 2] = 1.0
    nrm[3] = [np.nan, 0, 0]
    vm, got = _check_map(dev, [pts], [nrm], vgicp_ref.HAND_VOXEL, 0.5)
    assert got['keys'].tolist() == [vgicp_ref.key_of(c) for c in vgicp_ref.HAND_KEYS] and got['counts'].tolist() == vgicp_ref.HAND_COUNTS
    assert np.array_equal(got['covs'][2], [1, 0, 0, 1, 0, 0.75]) and np.array_equal(got['means'][1], [-0.1875, 0, 0])


def test_map_of_small_clouds_runs_and_lattices(dev):
    rng = np.random.default_rng(7)
    sc = vgicp_ref.scene()
    clouds = [sc['tgt'][:0], sc['tgt'][:1], sc['tgt'][:2]]                              # 0, 1 and 2 points
    normals = [sc['tgt_normals'][:0], sc['tgt_normals'][:1], sc['tgt_normals'][:2]]
    for n in (63, 64, 65, 1800):                                                         # all points in one voxel
        clouds.append(rng.uniform(0.21, 0.39, (n, 3)).astype(np.float32))
        normals.append(_unit(rng, n))
    g = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing='ij'), -1).reshape(-1, 3)   # every point its own voxel, shuffled
    clouds.append(((g[rng.permutation(len(g))] + 0.5) * V + rng.uniform(-0.05, 0.05, (len(g), 3))).astype(np.float32))
    normals.append(_unit(rng, len(g)))
    vm, got = _check_map(dev, clouds, normals, V)                                        # ... as eight clouds of one map
    cnt = [got['counts'][got['row_off'][c]:got['row_off'][c + 1]].tolist() for c in range(len(clouds))]
    assert cnt[:2] == [[], [1]] and sum(cnt[2]) == 2 and cnt[3:7] == [[63], [64], [65], [1800]] and cnt[7] == [1] * 125
    for c in (0, 1, 5, 7):                                                               # ... and alone: the same rows
        _, one = _check_map(dev, [clouds[c]], [normals[c]], V)
        lo, hi = got['row_off'][c], got['row_off'][c + 1]
        assert all(np.array_equal(one[k], got[k][lo:hi]) for k in ('keys', 'counts', 'means', 'covs'))


def test_map_without_normals_and_with_bad_normals(dev):
    sc = vgicp_ref.scene()
    _, none = _check_map(dev, [sc['tgt']], None, V)
    assert np.array_equal(none['covs'], np.tile([1.0, 0, 0, 1, 0, 1], (len(none['covs']), 1)))
    nrm = sc['tgt_normals'].copy()
    nrm[::5] = [np.nan, 0, 1]
    nrm[1::7] *= np.float32(1.5)
    nrm[3] = [np.inf, 0, 0]
    _check_map(dev, [sc['tgt']], [nrm], V)
    _, junk = _check_map(dev, [sc['tgt']], [np.full_like(nrm, np.nan)], V)
    assert all(np.array_equal(junk[k], none[k]) for k in none)                          # normals that all count as none: C = I


def test_three_clouds_in_one_call_equal_three_calls(dev):
    sc = vgicp_ref.scene()
    clouds, normals = [sc['tgt'], sc['tgt'][:1234], sc['src']], [sc['tgt_normals'], sc['tgt_normals'][:1234], sc['src_normals']]
    _, got = _check_map(dev, clouds, normals, V)
    for c in range(3):
        _, one = _check_map(dev, [clouds[c]], [normals[c]], V)
        lo, hi = got['row_off'][c], got['row_off'][c + 1]
        assert all(np.array_equal(one[k], got[k][lo:hi]) for k in ('keys', 'counts', 'means', 'covs')), c


# ---------------------------------------------------------------------------------------------------- the loop
# measured on an MI355X, max |T - restatement| after one step from the identity / from the start pose, and the larger of the
# |inlier_rmse - restatement| of the zero-iteration and one-step passes:
#   1 neighbour 2.27e-15 / 4.51e-16, rmse 5.55e-17;  7 neighbours 3.71e-15 / 2.01e-15, rmse 2.78e-17;  27 neighbours 2.07e-15 / 2.72e-15,
#   rmse 2.78e-17.  A few units in the last place: the two differ in the order of their sums, the 3x3 inverse and the 6x6 solve.
ONE_STEP_ATOL = {1: (4.6e-15, 1.2e-16), 7: (7.5e-15, 5.6e-17), 27: (5.5e-15, 5.6e-17)}      # (T, rmse)


@pytest.mark.parametrize("nb", [1, 7, 27])
@pytest.mark.parametrize("init", ["identity", "start"])
def test_zero_iterations_and_one_step_match_the_restatement(dev, scene_map, nb, init):
    sc = vgicp_ref.scene()
    dmap, rmap = scene_map
    T0 = None if init == "identity" else vgicp_ref.start()
    inits = None if T0 is None else [T0]
    want0 = vgicp_ref.vgicp(sc['src'], rmap, nb, sc['src_normals'], T0, 0)
    r0 = _scene_run(dev, dmap, nb, inits=inits, max_iteration=0)
    assert want0['terms'] >= 900 and (want0['rows'] >= 0).all()
    assert np.array_equal(r0['rows'], want0['rows'])
    assert r0['iterations'] == 0 and np.array_equal(r0['T'], np.eye(4) if T0 is None else T0)
    assert r0['fitness'] == want0['fitness'] == 1.0
    # the device's term count, recovered from its rmse = sqrt(sum d2 / terms) and the restatement's sum d2 (equal to a few ulp)
    terms = want0['terms'] * (want0['inlier_rmse'] / r0['inlier_rmse']) ** 2
    assert abs(terms - want0['terms']) < 1e-6, (terms, want0['terms'])
    print(f'MEASURED zero iterations ({nb}, {init}): |drmse| = {abs(r0["inlier_rmse"] - want0["inlier_rmse"]):.3g}')
    assert_close(r0['inlier_rmse'], want0['inlier_rmse'], 0.0, ONE_STEP_ATOL[nb][1], f'zero iterations rmse ({nb}, {init})')
    want1 = vgicp_ref.vgicp(sc['src'], rmap, nb, sc['src_normals'], T0, 1)
    r1 = _scene_run(dev, dmap, nb, inits=inits, max_iteration=1)
    assert r1['iterations'] == 1 and want1['iterations'] == 1
    print(f'MEASURED one step ({nb}, {init}): |dT| = {np.abs(r1["T"] - want1["T"]).max():.3g}, |drmse| = {abs(r1["inlier_rmse"] - want1["inlier_rmse"]):.3g}')
    assert_close(r1['T'], want1['T'], 0.0, ONE_STEP_ATOL[nb][0], f'one step T ({nb}, {init})')
    assert np.array_equal(r1['rows'], want1['rows']) and r1['fitness'] == want1['fitness']
    assert_close(r1['inlier_rmse'], want1['inlier_rmse'], 0.0, ONE_STEP_ATOL[nb][1], f'one step rmse ({nb}, {init})')


# measured on an MI355X, max |T - restatement| after the loop: 1.11e-16 (1 neighbour, 4 updates), 3.47e-17 (7, 5 updates), 1.11e-16 (27, 5 updates)
FULL_ATOL = {1: 2.3e-16, 7: 7e-17, 27: 2.3e-16}


@pytest.mark.parametrize("nb", [1, 7, 27])
def test_full_loop_matches_the_restatement_and_the_planted_pose(dev, scene_map, nb):
    sc = vgicp_ref.scene()
    dmap, rmap = scene_map
    want = vgicp_ref.vgicp(sc['src'], rmap, nb, sc['src_normals'], None, 50)
    r = _scene_run(dev, dmap, nb, max_iteration=50)
    assert r['iterations'] == want['iterations'] and 0 < r['iterations'] < 50
    assert np.array_equal(r['rows'], want['rows']) and r['fitness'] == want['fitness'] == 1.0
    print(f'MEASURED full loop ({nb}): |dT| = {np.abs(r["T"] - want["T"]).max():.3g}, |drmse| = {abs(r["inlier_rmse"] - want["inlier_rmse"]):.3g}')
    assert_close(r['T'], want['T'], 0.0, FULL_ATOL[nb], f'full loop T ({nb})')
    rot, tr = gicp_ref.pose_error(r['T'], sc['T'])
    print(f'device voxelized ICP, {nb} neighbours: {rot:.4f} deg, {tr * 1e3:.3f} mm from the planted pose in {r["iterations"]} updates')
    assert rot < 0.051 and tr < 0.92e-3                                   # the bound tests/test_vgicp_cpu.py puts on the restatement


_SIZES = [(0, 1800), (1, 1500), (255, 1700), (256, 1800), (257, 1234), (900, 1800)]


def test_batch_composition_and_reruns_give_the_same_bits(dev):
    from buffer_amd import icp
    sc = vgicp_ref.scene()
    S, SN = [_dev(sc['src'][:n], dev) for n, _ in _SIZES], [_dev(sc['src_normals'][:n], dev) for n, _ in _SIZES]
    Tg, TN = [_dev(sc['tgt'][:m], dev) for _, m in _SIZES], [_dev(sc['tgt_normals'][:m], dev) for _, m in _SIZES]
    kw = dict(voxel=V, max_iteration=40, return_rows=True)
    a = icp.vgicp_batched(S, Tg, src_normals=SN, tgt_normals=TN, **kw)
    b = icp.vgicp_batched(S, Tg, src_normals=SN, tgt_normals=TN, **kw)
    assert all(_same(x, y) for x, y in zip(a, b))
    for i in range(len(_SIZES)):
        one = icp.vgicp_batched([S[i]], [Tg[i]], src_normals=[SN[i]], tgt_normals=[TN[i]], **kw)[0]
        assert _same(one, a[i]), _SIZES[i]
    rev = icp.vgicp_batched(S[::-1], Tg[::-1], src_normals=SN[::-1], tgt_normals=TN[::-1], **kw)[::-1]
    assert all(_same(x, y) for x, y in zip(a, rev))
    assert a[0]['iterations'] == 0 and a[0]['fitness'] == 0.0 and np.array_equal(a[0]['T'], np.eye(4)) and a[0]['rows'].shape == (0,)
    assert a[1]['iterations'] == 0 and np.array_equal(a[1]['T'], np.eye(4)) and a[1]['fitness'] == 1.0    # 4 terms: no 6x6 system
    for i in range(2, len(_SIZES)):                                        # (margins: tests/test_vgicp_cpu.py, sub-cloud cases)
        n, m = _SIZES[i]
        want = vgicp_ref.vgicp(sc['src'][:n], vgicp_ref.build_map(sc['tgt'][:m], sc['tgt_normals'][:m], V), 7, sc['src_normals'][:n], None, 40)
        assert a[i]['iterations'] == want['iterations'] > 0 and np.array_equal(a[i]['rows'], want['rows']), _SIZES[i]


def test_shared_targets_and_a_reused_map(dev):
    from buffer_amd import icp
    sc = vgicp_ref.scene()
    S = [_dev(sc['src'][:n], dev) for n in (900, 257, 500, 700)]
    SN = [_dev(sc['src_normals'][:n], dev) for n in (900, 257, 500, 700)]
    Tg, TN = [_dev(sc['tgt'], dev), _dev(sc['tgt'][:1500], dev)], [_dev(sc['tgt_normals'], dev), _dev(sc['tgt_normals'][:1500], dev)]
    inits = [np.eye(4), vgicp_ref.start(), vgicp_ref.start(), np.eye(4)]
    kw = dict(src_normals=SN, inits=inits, neighbors=27, max_iteration=40, return_rows=True)
    shared_map = icp.voxel_map(Tg, V, TN)
    shared = icp.vgicp_batched(S, shared_map, pair_target=[0, 1, 0, 1], **kw)
    own = icp.vgicp_batched(S, [Tg[0], Tg[1], Tg[0], Tg[1]], tgt_normals=[TN[0], TN[1], TN[0], TN[1]], voxel=V, **kw)
    assert all(_same(x, y) for x, y in zip(shared, own)) and all(r['iterations'] > 0 for r in shared)
    again = icp.vgicp_batched(S, shared_map, pair_target=[0, 1, 0, 1], **kw)           # the map built once, a second call on it
    fresh = icp.vgicp_batched(S, icp.voxel_map(Tg, V, TN), pair_target=[0, 1, 0, 1], **kw)
    assert all(_same(x, y) for x, y in zip(shared, again)) and all(_same(x, y) for x, y in zip(shared, fresh))
    swapped = icp.vgicp_batched(S[:2], shared_map, pair_target=[1, 0], **dict(kw, src_normals=SN[:2], inits=inits[:2]))
    assert not np.array_equal(swapped[0]['T'], shared[0]['T'])                         # pair_target does choose the cloud


def test_edge_rows(dev, scene_map):
    from buffer_amd import icp
    sc = vgicp_ref.scene()
    dmap, rmap = scene_map
    src = sc['src'].copy()
    src[::7] = np.nan
    src[3] = [np.inf, 0, 0]
    src[5] = [1e30, 0, 0]
    bad = np.flatnonzero(~np.isfinite(src).all(1) | (np.abs(src) > 1e20).any(1))
    r = icp.vgicp_batched([_dev(src, dev)], dmap, src_normals=[_dev(sc['src_normals'], dev)], max_iteration=50, return_rows=True)[0]
    want = vgicp_ref.vgicp(src, rmap, 7, sc['src_normals'], None, 50)
    assert (r['rows'][bad] == -1).all() and np.array_equal(r['rows'], want['rows'])
    assert r['iterations'] == want['iterations'] > 0 and r['fitness'] == want['fitness'] == (900 - len(bad)) / 900
    far = icp.vgicp_batched([_dev(sc['src'] + np.float32(50.0), dev)], dmap, inits=[vgicp_ref.start()], return_rows=True)[0]
    assert far['fitness'] == 0.0 and far['inlier_rmse'] == 0.0 and far['iterations'] == 0 and (far['rows'] == -1).all()
    assert np.array_equal(far['T'], vgicp_ref.start())
    S, SN = _dev(sc['src'], dev), _dev(sc['src_normals'], dev)
    none = icp.vgicp_batched([S], dmap, max_iteration=50)[0]                             # src_normals=None: C = I on the source side
    zero = icp.vgicp_batched([S], dmap, src_normals=[torch.zeros_like(SN)], max_iteration=50)[0]
    wantn = vgicp_ref.vgicp(sc['src'], rmap, 7, None, None, 50)
    assert _same(none, zero) and none['iterations'] == wantn['iterations'] > 0
    Tg, TN = _dev(sc['tgt'], dev), _dev(sc['tgt_normals'], dev)
    e1 = icp.vgicp_batched([S], [Tg], src_normals=[SN], tgt_normals=[TN], voxel=V, epsilon=1.0, max_iteration=50)[0]
    iso = icp.vgicp_batched([S], [Tg], voxel=V, max_iteration=50)[0]
    assert _same(e1, iso) and e1['iterations'] > 0                                       # epsilon = 1: every covariance is I
    T0 = vgicp_ref.start()
    r = icp.vgicp_batched([S, S[:0]], [Tg[:0], Tg], inits=[T0, T0], voxel=V, src_normals=[SN, SN[:0]], tgt_normals=[TN[:0], TN], return_rows=True)
    assert all(np.array_equal(x['T'], T0) and x['fitness'] == 0.0 and x['iterations'] == 0 for x in r) and (r[0]['rows'] == -1).all()
    T, fit, rmse, rows = icp.icp_voxelized(S, SN, Tg, TN, V, max_iteration=50)           # the one-pair form
    full = _scene_run(dev, dmap, 7, max_iteration=50)
    assert np.array_equal(T, full['T']) and fit == full['fitness'] and rmse == full['inlier_rmse'] and np.array_equal(rows, full['rows'])


def test_terms_on_one_line_are_not_positive_definite(dev):
    """dyadic points on the x axis, every covariance I: H[0][0] (rotation about the line) is a sum of exact zeros in any order"""
    from buffer_amd import icp
    pts = np.zeros((8, 3), np.float32)
    pts[:, 0] = 0.125 + 0.25 * np.arange(8)
    rmap = vgicp_ref.build_map(pts, None, 0.25, 1.0)
    want = vgicp_ref.vgicp(pts, rmap, 7, None, None, 30)
    assert want['terms'] == 8 + 2 * 7 and not want['solvable'] and want['iterations'] == 0
    r = icp.vgicp_batched([_dev(pts, dev)], [_dev(pts, dev)], voxel=0.25, epsilon=1.0, return_rows=True)[0]
    assert r['iterations'] == 0 and np.array_equal(r['T'], np.eye(4)) and r['fitness'] == 1.0 and r['rows'].tolist() == list(range(8))
    assert r['inlier_rmse'] == want['inlier_rmse'] == np.sqrt(14 * 0.0625 / 22)         # dyadic sums are exact in any order


# ---------------------------------------------------------------------------------------------------- C ABI
def test_error_returns(dev, scene_map):
    from buffer_amd import _lib
    lib = _lib.lib()
    fake, null = C.c_void_p(0x1000), C.c_void_p(0)
    m = _lib.buf_voxel_map_t()

    def build(voxel=0.2, epsilon=1e-3, lengths=(10, 20)):
        ln = np.array(lengths, np.int32)
        rc = lib.buf_voxel_map_build(C.byref(m), fake, null, C.c_void_p(ln.ctypes.data), len(ln), voxel, epsilon, 1 << 16, fake, 16, fake, 16, null)
        return rc, lib.buf_last_error().decode()
    for v in (0.0, -0.2, float('nan'), float('inf')):
        rc, msg = build(voxel=v)
        assert rc == -1 and "voxel" in msg
    for e in (0.0, -1e-3, 1.0000001, float('nan'), float('inf')):
        rc, msg = build(epsilon=e)
        assert rc == -1 and "epsilon" in msg
    rc, msg = build(lengths=(10, -1))
    assert rc == -1 and "negative" in msg
    rc, msg = build()
    assert rc == -3 and "buffer" in msg                                    # well-formed arguments reach the size check
    dm = scene_map[0].m

    def run(neighbors=7, lengths=(10,), pair_cloud=None, mp=dm):
        ln = np.array(lengths, np.int32)
        pc = None if pair_cloud is None else np.array(pair_cloud, np.int32)
        rc = lib.buf_vgicp_batched(C.byref(mp), fake, null, C.c_void_p(ln.ctypes.data), null if pc is None else C.c_void_p(pc.ctypes.data),
                                   len(ln), neighbors, fake, 30, 1e-6, 1e-6, fake, fake, fake, fake, null, fake, 16, null)
        return rc, lib.buf_last_error().decode()
    for nb in (0, 2, 6, 8, 26, 28, -1):
        rc, msg = run(neighbors=nb)
        assert rc == -1 and "neighbors" in msg
    for pc in ([1], [-1]):
        rc, msg = run(pair_cloud=pc)
        assert rc == -1 and "pair_cloud" in msg
    rc, msg = run(lengths=(10, 10))                                       # two pairs, one map cloud, no pair_cloud
    assert rc == -1 and "pair_cloud" in msg
    rc, msg = run(lengths=(-1,))
    assert rc == -1 and "negative" in msg
    rc, msg = run(mp=_lib.buf_voxel_map_t())
    assert rc == -1 and "map" in msg
    rc, msg = run(pair_cloud=[0])
    assert rc == -3 and "workspace" in msg
    with pytest.raises(_lib.BufferHipError, match="max_cells"):            # BUF_ECAPACITY: the scene's box has 6 x 6 x 6 voxels
        from buffer_amd import ops
        sc = vgicp_ref.scene()
        ops.voxel_map_build(_dev(sc['tgt'], dev), [1800], V, max_cells=100)
    small = lib.buf_voxel_map_export(C.byref(dm), dm.nrows - 1, fake, fake, fake, fake, fake, null)
    assert small == -1 and "capacity" in lib.buf_last_error().decode()


def test_the_other_methods_keep_their_bits(dev, before_voxelized, scene_map):
    call, before = before_voxelized
    _scene_run(dev, scene_map[0], 27, max_iteration=5)
    for k, f in call.items():
        after = f()
        assert all(_same(x, y) for x, y in zip(before[k], after)), k
        assert all(r['iterations'] > 0 for r in after), k
