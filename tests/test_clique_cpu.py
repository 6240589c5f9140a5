"""The float64 restatement of N10 (tests/clique_ref.py) pinned on the CPU: its core numbers against the definition, its cliques, the
GNC case, its robustness down to 2 % true rows (where tests/sc2_ref.py fails), the margin conditions of every input that
tests/test_clique_gpu.py compares exactly, and the part of the surface that needs no device (CliqueOptions, exported symbols, the
size function, every BUF_EINVAL, the drivers' --estimator)."""
import ctypes as C

import numpy as np
import pytest

import clique_cases
import clique_ref
import fgr_cases
import sc2_cases
import sc2_ref

THR = clique_cases.THR
BUF_EINVAL = -1


def _graph(src, tgt, corr, d_thr):
    P, Q, live = sc2_ref.rows_of(src, tgt, corr)
    e = np.abs(sc2_ref.distances(P) - sc2_ref.distances(Q))
    Cm = (e <= d_thr) & live[:, None] & live[None, :]
    np.fill_diagonal(Cm, False)
    return Cm, live


def _cores_by_definition(Cm, live):
    """core_i = the largest k such that i survives when vertices of degree < k are removed until none is left"""
    core = np.full(len(Cm), -1)
    for k in range(len(Cm) + 1):
        keep = live.copy()
        while True:
            low = keep & ((Cm & keep[None, :]).sum(1) < k)
            if not low.any():
                break
            keep &= ~low
        if not keep.any():
            break
        core[keep] = k
    return core


@pytest.mark.parametrize('name', ['n4', 'n63', 'n64', 'n65', 'n65_dead_dup', 'n65_d0.1', 'n65_d10', 'n65_d1e-9'])
def test_core_numbers_against_the_definition(name):
    src, tgt, corr, opts, want = clique_cases.exact_case(name)
    Cm, live = _graph(src, tgt, corr, opts.get('d_thr', THR))
    assert np.array_equal(want['core'], _cores_by_definition(Cm, live))
    assert np.array_equal(want['deg'], np.where(live, Cm.sum(1), -1))
    assert want['info'][2] == (want['core'].max() + 1 if live.any() else 0)


def test_core_numbers_of_random_graphs():
    rng = np.random.default_rng(5)
    for n, p in ((1, 0.5), (7, 0.5), (33, 0.2), (65, 0.1), (65, 0.6)):
        A = np.triu(rng.random((n, n)) < p, 1)
        A = A | A.T
        live = rng.random(n) < 0.9
        A &= live[:, None] & live[None, :]
        assert np.array_equal(clique_ref.core_numbers(A, live), _cores_by_definition(A, live))


@pytest.mark.parametrize('name', [c[0] for c in clique_cases.EXACT_CASES])
def test_cliques_and_margin_conditions(name):
    """every input that the GPU tests compare exactly: a clique is a clique and no larger than the bound, the order is the stated one,
    and no decision lies within 1e-9 of its threshold (an input that violates a condition is replaced by the next draw of its
    sequence, never excused)"""
    src, tgt, corr, opts, want = clique_cases.exact_case(name)
    m = want['margins']
    print(f'clique margins {name}: info {want["info"].tolist()}, ' + ', '.join(f'{k} {v:.3e}' for k, v in m.items()))
    assert clique_cases.margins_hold(m)
    Cm, live = _graph(src, tgt, corr, opts.get('d_thr', THR))
    mem = want['members'][want['members'] >= 0]
    status, n_live, bound, size, rank, K, steps, count = want['info'].tolist()
    assert len(mem) == K == min(size, dict(clique_ref.DEFAULTS, **opts)['max_members']) and size <= bound and n_live == live.sum()
    assert Cm[np.ix_(mem, mem)].sum() == K * (K - 1) and len(set(mem.tolist())) == K
    order = np.argsort(want['rank'][live], kind='stable')
    keys = [(-want['core'][i], -want['deg'][i], i) for i in np.flatnonzero(live)[order]]
    assert keys == sorted(keys) and (want['rank'][~live] == -1).all() and (want['core'][~live] == -1).all()
    n = len(corr)
    if n < 3 or 'd1e-9' in name:
        assert status == clique_ref.NOTHING and np.array_equal(want['T'], np.eye(4)) and count == 0 and not want['inliers'].any()
    if 'd1e-9' in name:
        assert bound == 1 and size == 1 and (want['deg'] == 0).all()
    if 'd10' in name:
        assert size == bound == n and K == min(n, 256) and (want['sizes'][:64] == n).all()
    if 'd0.1' in name:
        assert bound >= size and status == clique_ref.OK and (steps > 1 or n < 129)   # (false rows in the clique: GNC engaged)
    if 'members16' in name:
        assert K == 16 < size
    if 'seeds1' in name:
        assert (want['sizes'][1:] == -1).all() and rank == 0
    if 'dead_dup' in name:
        assert n_live == n - len({0, 63, 64, n - 1}) and not np.isin([0, 63, 64, n - 1], mem).any()
    if n >= 63 and 'd1e-9' not in name:
        assert status == clique_ref.OK and count >= 3


def test_margin_conditions_of_the_larger_input():
    want = clique_cases.large_case()[3]
    print(f'clique margins rows3000: info {want["info"].tolist()}, peel levels {want["peel_levels"]}, '
          + ', '.join(f'{k} {v:.3e}' for k, v in want['margins'].items()))
    assert clique_cases.margins_hold(want['margins'])
    assert want['info'][3] == want['info'][2] > 2000 and want['info'][5] == 256 and want['certified']


def test_gnc_case():
    src, tgt, corr, opts, T, want = clique_cases.gnc_case()
    w = want['weights'][:1128]
    a, b = np.triu_indices(48, 1)
    m = want['members'][:48]
    false_tim = (m[a] >= 40) | (m[b] >= 40)                      # rows 40..47 of this input are the false ones
    rre, _ = fgr_cases.errors(want['T'], T)
    print(f'clique GNC case: info {want["info"].tolist()}, zeros {int((w == 0).sum())}, ones {int((w == 1).sum())}, {rre:.3e} deg, margins '
          + ', '.join(f'{k} {v:.3e}' for k, v in want['margins'].items()))
    assert clique_cases.margins_hold(want['margins'])
    assert want['info'][3] == want['info'][2] == 48 and want['info'][5] == 48 and np.isnan(want['weights'][1128:]).all()
    assert false_tim.sum() == 348 and np.array_equal(w == 0.0, false_tim) and np.array_equal(w == 1.0, ~false_tim)
    assert rre <= 0.1
    one = clique_ref.clique(src, tgt, corr, opts['d_thr'], tim_thr=0.03, refine_iterations=0, gnc_iterations=1)
    assert one['info'][6] == 1 and fgr_cases.errors(one['T'], T)[0] > rre


@pytest.mark.parametrize('true_rows,case', clique_cases.ROBUST)
def test_restatement_is_robust(true_rows, case):
    src, tgt, corr, T, want = clique_cases.robust_case(true_rows, case)
    rre, rte = fgr_cases.errors(want['T'], T)
    print(f'clique restatement, {true_rows} true rows of 300, case {case}: info {want["info"].tolist()}, certified {want["certified"]}, '
          f'{rre:.3e} deg, {rte:.3e}, margins ' + ', '.join(f'{k} {v:.3e}' for k, v in want['margins'].items()))
    assert clique_cases.margins_hold(want['margins'])            # the GPU test compares these inputs exactly as well
    assert want['info'][0] == clique_ref.OK
    if true_rows == 6:
        assert rre <= 1.0 and rte <= 0.02 and not want['certified']
    else:
        assert rre <= 0.15 and rte <= 0.0025 and want['certified']


def test_sc2_fails_where_the_clique_holds():
    """six true rows of 300: the SC2 restatement is more than a degree off (or finds nothing) on at least three of the six cases"""
    off = 0
    for case in range(6):
        src, tgt, corr, T = sc2_cases.low_inlier_case(6, case)
        out = sc2_ref.sc2(src, tgt, corr, THR, THR)
        off += int(out['info'][0] == sc2_ref.NOTHING or fgr_cases.errors(out['T'], T)[0] > 1.0)
    assert off >= 3, off


def test_options_map_onto_the_kernel_arguments():
    from buffer_amd.clique import CliqueOptions
    o = CliqueOptions()
    assert o.kernel_arguments() == dict(d_thr=0.1, tim_thr=0.1, t_thr=0.05, inlier_thr=0.1, max_seeds=64, max_members=256, gnc_factor=1.4,
                                        gnc_iterations=100, refine_iterations=20)
    assert {k: v for k, v in o.kernel_arguments().items() if not k.endswith('_thr')} == clique_ref.DEFAULTS
    k = CliqueOptions(d_thr=0.0375, tim_thr=0.05, t_thr=0.01, max_members=40).kernel_arguments()
    assert (k['d_thr'], k['tim_thr'], k['t_thr'], k['inlier_thr'], k['max_members']) == (0.0375, 0.05, 0.01, 0.0375, 40)
    assert CliqueOptions(d_thr=0.03).t_thr == 0.015 and 'max_seeds=64' in repr(o)


def test_estimator_option(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--estimator', 'clique'])
        assert a.descriptor == 'fpfh' and a.estimator == 'clique'
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['--root', 'r', '--estimator', 'clique'])
        assert e.value.code == 2 and '--descriptor fpfh' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--estimator', 'teaser'])
        assert mod.parse_args(['--root', 'r'])[0].estimator == 'ransac'
    from buffer_amd import fpfh
    assert fpfh.ESTIMATORS == ('ransac', 'fgr') and fpfh.ALL_ESTIMATORS == ('ransac', 'fgr', 'sc2')
    assert fpfh.KNOWN_ESTIMATORS == ('ransac', 'fgr', 'sc2', 'clique')


def test_header_and_symbols():
    import os
    from buffer_amd import _lib, build
    build.build()
    assert {'buf_clique_batched', 'buf_clique_ws_bytes'} <= set(_lib.exported_symbols())
    assert _lib.lib().buf_version() == 670
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'buffer_hip.h')).read()
    for word in ('buf_clique_batched', 'buf_clique_ws_bytes', 'BUF_CLIQUE_NOTHING', 'BUF_CLIQUE_OK', 'N10', 'unpinned'):
        assert word in header, word


def test_workspace_size():
    from buffer_amd import _lib
    L = _lib.lib()
    hp = lambda a: C.c_void_p(a.ctypes.data)
    lens = lambda *v: np.array(v, np.int32)
    f = lambda a, ms=64, mm=256, B=None: int(L.buf_clique_ws_bytes(hp(a), len(a) if B is None else B, ms, mm))
    assert 0 < f(lens(0)) <= f(lens(1)) < f(lens(300)) < f(lens(3000)) < f(lens(16384))
    assert f(lens(300)) < f(lens(300, 300)) and f(lens(300), ms=64) < f(lens(300), ms=65) and f(lens(300), mm=256) < f(lens(300), mm=257)
    assert f(lens(300)) < 1 << 20                                # sized from the actual lengths, not from the limit
    for bad in (dict(ms=0), dict(ms=1025), dict(mm=2), dict(mm=513), dict(B=0), dict(B=65536)):
        assert f(lens(300), **bad) == 0, bad
    assert f(lens(16385)) == 0 and f(lens(-1)) == 0 and int(L.buf_clique_ws_bytes(None, 1, 64, 256)) == 0


DEFAULT_TAIL = dict(d_thr=THR, tim_thr=THR, t_thr=THR / 2, inlier_thr=THR, max_seeds=64, max_members=256, gnc_factor=1.4,
                    gnc_iterations=100, refine_iterations=20)
BAD = [dict(d_thr=0.0), dict(d_thr=-1.0), dict(d_thr=float('nan')), dict(d_thr=float('inf')), dict(tim_thr=0.0), dict(tim_thr=1e200),
       dict(tim_thr=1e-200), dict(tim_thr=float('nan')), dict(t_thr=0.0), dict(t_thr=float('inf')), dict(t_thr=1e200),
       dict(inlier_thr=0.0), dict(inlier_thr=-1.0), dict(inlier_thr=float('inf')), dict(max_seeds=0), dict(max_seeds=1025),
       dict(max_members=2), dict(max_members=513), dict(gnc_factor=1.0), dict(gnc_factor=float('inf')), dict(gnc_factor=float('nan')),
       dict(gnc_iterations=0), dict(gnc_iterations=1001), dict(refine_iterations=-1)]


def test_every_einval_without_a_device():
    """the argument checks come before any device work: host memory stands in for every device pointer and stays untouched"""
    from buffer_amd import _lib
    L = _lib.lib()
    hp = lambda a: C.c_void_p(a.ctypes.data)
    one, neg, big = np.array([1], np.int32), np.array([-1], np.int32), np.array([16385], np.int32)
    buf = np.zeros(1 << 12, np.float64)

    def call(npairs=1, lens=(one, one, one), null=(), ws_bytes=(1 << 12) * 8, **opts):
        o = dict(DEFAULT_TAIL, **opts)
        p = dict(src=hp(buf), sl=hp(lens[0]), tgt=hp(buf), tl=hp(lens[1]), corr=hp(buf), cl=hp(lens[2]), T=hp(buf), info=hp(buf), ws=hp(buf))
        for k in null:
            p[k] = None
        return L.buf_clique_batched(p['src'], p['sl'], p['tgt'], p['tl'], p['corr'], p['cl'], npairs, o['d_thr'], o['tim_thr'], o['t_thr'],
                                    o['inlier_thr'], o['max_seeds'], o['max_members'], o['gnc_factor'], o['gnc_iterations'],
                                    o['refine_iterations'], p['T'], p['info'], None, None, None, None, None, None, None, None, p['ws'],
                                    ws_bytes, None)

    for opts in BAD:
        assert call(**opts) == BUF_EINVAL, opts
        assert call(npairs=0, **opts) == BUF_EINVAL, opts         # the parameters are checked even where there is nothing to do
    for null in ('sl', 'tl', 'cl', 'T', 'info', 'ws', 'src', 'tgt', 'corr'):
        assert call(null=(null,)) == BUF_EINVAL, null
    for lens in ((neg, one, one), (one, neg, one), (one, one, neg), (one, one, big)):
        assert call(lens=lens) == BUF_EINVAL
    assert call(npairs=-1) == BUF_EINVAL and call(npairs=65536) == BUF_EINVAL
    need = int(L.buf_clique_ws_bytes(hp(one), 1, 64, 256))
    assert call(ws_bytes=need - 1) == BUF_EINVAL and b'workspace' in L.buf_last_error()
    assert call(npairs=0, null=('sl', 'tl', 'cl', 'T', 'info', 'ws', 'src', 'tgt', 'corr'), ws_bytes=0) == 0   # nothing to do: accepted
    assert (buf == 0).all()
