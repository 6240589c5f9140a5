"""buf_fgr_batched (csrc/fgr.hip: k_fgr_tuples, k_fgr_optimize) through its C entry point against the float64 restatement
tests/fgr_ref.py (pinned by tests/test_fgr_cpu.py).

The tuple list is a chain of exact decisions (integer draws, IEEE products and comparisons in fp64): rows_out, the tuple count and
the trials examined are compared with array_equal.  The optimisation runs the restatement's operations with sums of another shape
(256 lanes and a tree against numpy's), so poses and weights are compared within limits of twice what was measured on an MI355X over
ALL optimisation cases of this file (each case prints its own figures before it asserts):
    max |T - T_ref| = 7.772e-16 (rows255),  max |w - w_ref| = 2.220e-15 (the two delta_absolute cases)
on unit-scale data: a few ulp, far inside the 1e-9 that would be a finding.  By case, |dT| / |dw|: rows12 5.6e-16 / 4.4e-16, rows255
7.8e-16 / 8.9e-16, rows258_it5 2.2e-16 / 4.4e-16, rows3000 3.3e-16 / 4.4e-16, rows258_it1 2.2e-16 / 0, rows3000_absolute 3.3e-16 /
2.2e-15, rows255_every1 2.2e-16 / 4.4e-16, rows258_absolute 4.4e-16 / 2.2e-15; rows9, rows258_it0 and cloud1 are exact.
Status, tuple count and update count must be equal.  Outputs are prefilled with NaN / -2 and carry guard words past their end.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fgr_cases
import fgr_ref

pytestmark = pytest.mark.gpu
BUF_EINVAL = -1
GUARD = 64
MEASURED_DT = 7.8e-16
MEASURED_DW = 2.3e-15
DEFAULTS = dict(tuple_scale=0.95, max_tuples=1000, trial_factor=100, mu_start=1.0, delta=0.025, delta_absolute=0, division_factor=1.4,
                decrease_every=4, iterations=64)


def _lib():
    from buffer_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_call(dev, pairs, opts, want_rows=True, ws_short=0, expect=0, null=()):
    """pairs: list of (src f32[ns,3], tgt f32[nt,3], corr int[n,2], seed) -> the raw guarded output buffers after one call"""
    L = _lib()
    o = dict(DEFAULTS, **opts)
    B, mt = len(pairs), int(o['max_tuples'])
    cat = lambda k, w, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(
        [np.asarray(p[k], dt).reshape(-1, w) for p in pairs] + [np.zeros((0, w), dt)]))).to(dev)
    src, tgt, corr = cat(0, 3, np.float32), cat(1, 3, np.float32), cat(2, 2, np.int32)
    sl, tl, cl = (np.array([len(np.asarray(p[k]).reshape(-1, w)) for p in pairs], np.int32) for k, w in ((0, 3), (1, 3), (2, 2)))
    seeds = np.array([p[3] for p in pairs], np.uint64)
    mtc = max(mt, 1) if 1 <= mt <= 4096 else 1
    T = torch.full((B * 16 + GUARD,), float('nan'), dtype=torch.float64, device=dev)
    info = torch.full((B * 4 + GUARD,), -2, dtype=torch.int32, device=dev)
    rows = torch.full((B * 6 * mtc + GUARD,), -2, dtype=torch.int32, device=dev)
    wts = torch.full((B * 3 * mtc + GUARD,), float('nan'), dtype=torch.float64, device=dev)
    wts[:B * 3 * mtc] = -2.0
    nbytes = int(L.buf_fgr_ws_bytes(int(corr.shape[0]), B, mt))
    ws = torch.zeros((max(nbytes, 8) + 8 * GUARD,), dtype=torch.uint8, device=dev)
    ws[nbytes:] = 0xA5
    hp = lambda a: C.c_void_p(a.ctypes.data)
    args = dict(src=_p(src), sl=hp(sl), tgt=_p(tgt), tl=hp(tl), corr=_p(corr), cl=hp(cl), seeds=hp(seeds), T=_p(T), info=_p(info),
                rows=_p(rows) if want_rows else None, wts=_p(wts) if want_rows else None, ws=_p(ws))
    for k in null:
        args[k] = None
    rc = L.buf_fgr_batched(args['src'], args['sl'], args['tgt'], args['tl'], args['corr'], args['cl'], B, args['seeds'],
                           float(o['tuple_scale']), mt, int(o['trial_factor']), float(o['mu_start']), float(o['delta']),
                           int(o['delta_absolute']), float(o['division_factor']), int(o['decrease_every']), int(o['iterations']),
                           args['T'], args['info'], args['rows'], args['wts'], args['ws'], max(nbytes - ws_short, 0), _stream())
    assert rc == expect, (rc, L.buf_last_error())
    torch.cuda.synchronize()
    assert (ws[nbytes:].cpu().numpy() == 0xA5).all(), 'write past the end of the workspace'
    return dict(T=T.cpu().numpy(), info=info.cpu().numpy(), rows=rows.cpu().numpy(), wts=wts.cpu().numpy(), B=B, mt=mtc)


def _untouched(raw, want_rows=True):
    B, mt = raw['B'], raw['mt']
    ok = np.isnan(raw['T']).all() and (raw['info'] == -2).all()
    if want_rows:
        ok = ok and (raw['rows'] == -2).all() and (raw['wts'][:B * 3 * mt] == -2.0).all() and np.isnan(raw['wts'][B * 3 * mt:]).all()
    return bool(ok)


def _call(dev, pairs, want_rows=True, **opts):
    """-> per pair dict(T f64[4,4], info int32[4], rows int32[3 mt, 2], weights f64[3 mt]); every value written, the guards untouched"""
    raw = _raw_call(dev, pairs, opts, want_rows)
    B, mt = raw['B'], raw['mt']
    assert np.isnan(raw['T'][B * 16:]).all() and (raw['info'][B * 4:] == -2).all(), 'write past the end'
    assert (raw['rows'][B * 6 * mt:] == -2).all() and np.isnan(raw['wts'][B * 3 * mt:]).all(), 'write past the end'
    assert not np.isnan(raw['T'][:B * 16]).any() and not (raw['info'][:B * 4] == -2).any(), 'a value was not written'
    if want_rows:
        assert not (raw['rows'][:B * 6 * mt] == -2).any() and not (raw['wts'][:B * 3 * mt] == -2.0).any(), 'a value was not written'
    else:
        assert (raw['rows'] == -2).all() and (raw['wts'][:B * 3 * mt] == -2.0).all()
    return [dict(T=raw['T'][16 * b:16 * b + 16].reshape(4, 4).copy(), info=raw['info'][4 * b:4 * b + 4].copy(),
                 rows=raw['rows'][6 * mt * b:6 * mt * (b + 1)].reshape(-1, 2).copy(), weights=raw['wts'][3 * mt * b:3 * mt * (b + 1)].copy())
            for b in range(B)]


@functools.lru_cache(maxsize=None)
def _pair(seed, n, ncorr=None, noise=0.002, false_frac=0.2):
    """cloud of n points and its moved, noisy copy; ncorr (default n) identity matches of which false_frac go astray"""
    src, tgt, _ = fgr_cases.moved_cloud(seed, n, noise)
    m = n if ncorr is None else ncorr
    rng = np.random.default_rng(seed + 1000)
    corr = np.stack([np.arange(m) % n, np.arange(m) % n], 1).astype(np.int32)
    bad = rng.random(m) < false_frac
    corr[bad, 1] = rng.integers(0, n, int(bad.sum()))
    return src, tgt, corr


def _same(a, b):
    return (np.array_equal(a['T'], b['T']) and np.array_equal(a['info'], b['info']) and np.array_equal(a['rows'], b['rows'])
            and np.array_equal(a['weights'], b['weights'], equal_nan=True))


# ------------------------------------------------------------------------------------------ the tuple list, exact
# (name, cloud n, correspondences, options, what to inject)
TUPLE_CASES = [('n1', 40, 1, {}, None), ('n2', 40, 2, {}, None), ('n3', 40, 3, {}, None), ('n7', 40, 7, {}, None),
               ('n300_cap37', 300, 300, dict(max_tuples=37), None), ('n300_cap1000', 300, 300, {}, None),
               ('n300_budget', 300, 300, dict(tuple_scale=0.9999), None), ('n300_bad_index_nan', 300, 300, {}, 'bad')]


@pytest.mark.parametrize('name,n,ncorr,opts,inject', TUPLE_CASES, ids=[c[0] for c in TUPLE_CASES])
def test_tuple_list_is_exact(dev, name, n, ncorr, opts, inject):
    # (n300_budget: target noise 2e-4, so that the edge ratios stay within 1 - 0.9999 for some trials and not for most)
    src, tgt, corr = _pair(21, n, ncorr, noise=2e-4 if name == 'n300_budget' else 0.002,
                           false_frac=0.0 if name in ('n1', 'n2', 'n3', 'n7') else 0.2)
    src, corr = src.copy(), corr.copy()
    if inject:
        corr[17, 1] = n                                          # one row past the end of the target cloud
        corr[18, 0] = -1
        src[33, 2] = np.nan                                      # one NaN point
    want = fgr_ref.fgr(src, tgt, corr, 5, **dict(DEFAULTS, **opts))
    got = _call(dev, [(src, tgt, corr, 5)], **opts)[0]
    print(f'FGR tuples {name}: kept {got["info"][1]} (ref {want["info"][1]}), trials {got["info"][2]} (ref {want["info"][2]})')
    assert np.array_equal(got['info'][1:3], want['info'][1:3]), (got['info'], want['info'])
    assert np.array_equal(got['rows'], want['rows']), int((got['rows'] != want['rows']).sum())
    mt = dict(DEFAULTS, **opts)['max_tuples']
    if name in ('n1', 'n2'):
        assert got['info'][1] == 0 and got['info'][2] == 100 * ncorr                 # a repeated index rejects every trial
    if name == 'n3':
        assert 0 < got['info'][1] < 300
    if name == 'n7':
        assert got['info'][2] == 700
    if name.startswith('n300_cap'):
        assert got['info'][1] == mt and got['info'][2] < 30000
    if name == 'n300_cap37':
        assert got['info'][2] % 256 not in (0, 255)              # the list filled inside a chunk of trials
    if name == 'n300_budget':
        assert 0 < got['info'][1] < mt and got['info'][2] == 30000
    if inject:
        kept = got['rows'][:3 * got['info'][1]]
        assert got['info'][1] == mt and not ((kept[:, 0] == 33) | (kept[:, 0] < 0) | (kept[:, 1] >= n)).any()


# ------------------------------------------------------------------------------------------ the optimisation against the restatement
# (name, cloud n, options): the kept list has 3 * max_tuples rows (the cap is reached in every case but cloud1)
OPT_CASES = [('rows9', 255, dict(max_tuples=3)), ('rows12', 257, dict(max_tuples=4)), ('rows255', 255, dict(max_tuples=85)),
             ('rows258_it5', 257, dict(max_tuples=86, iterations=5)), ('rows3000', 2000, {}),
             ('rows258_it0', 257, dict(max_tuples=86, iterations=0)), ('rows258_it1', 257, dict(max_tuples=86, iterations=1)),
             ('rows3000_absolute', 2000, dict(delta=0.05, delta_absolute=1)), ('rows255_every1', 255, dict(max_tuples=85, decrease_every=1)),
             ('rows258_absolute', 257, dict(max_tuples=86, delta=0.05, delta_absolute=1)), ('cloud1', 1, {})]


@pytest.mark.parametrize('name,n,opts', OPT_CASES, ids=[c[0] for c in OPT_CASES])
def test_optimisation_matches_the_restatement(dev, name, n, opts):
    src, tgt, corr = _pair(31, n)
    want = fgr_ref.fgr(src, tgt, corr, 9, **dict(DEFAULTS, **opts))
    got = _call(dev, [(src, tgt, corr, 9)], **opts)[0]
    m = 3 * int(want['info'][1])
    dT = float(np.abs(got['T'] - want['T']).max())
    dw = float(np.abs(got['weights'][:m] - want['weights'][:m]).max()) if m and not np.isnan(want['weights'][:m]).all() else 0.0
    print(f'FGR optimisation {name}: info {got["info"].tolist()} (ref {want["info"].tolist()}), max |dT| = {dT:.3e}, max |dw| = {dw:.3e}')
    assert np.array_equal(got['info'], want['info']), (got['info'], want['info'])
    assert np.array_equal(got['rows'], want['rows'])
    assert np.array_equal(np.isnan(got['weights']), np.isnan(want['weights']))
    assert dT <= 2 * MEASURED_DT and dw <= 2 * MEASURED_DW, (dT, dw)
    mt, it = dict(DEFAULTS, **opts)['max_tuples'], dict(DEFAULTS, **opts)['iterations']
    if name == 'cloud1':
        assert got['info'].tolist() == [fgr_ref.NOTHING, 0, 100, 0]
    elif name == 'rows9':
        assert got['info'].tolist()[:2] == [fgr_ref.NOTHING, 3] and got['info'][3] == 0 and np.array_equal(got['T'], np.eye(4))
    else:
        assert got['info'][0] == fgr_ref.OK and got['info'][1] == mt and got['info'][3] == it
        if it == 0:
            assert np.array_equal(got['T'], np.eye(4)) and np.isnan(got['weights']).all()
        elif m == 3000:                                          # (false rows among 1000 tuples: some weights near 0)
            assert 0.0 < np.nanmin(got['weights']) < 0.5 and np.nanmax(got['weights']) > 0.9      # the line process is at work


def test_degenerate_systems(dev):
    # one correspondence repeated: every edge is 0, the strict tuple test keeps nothing (so such a list never reaches the solver)
    src, tgt, _ = _pair(31, 255)
    got = _call(dev, [(src, tgt, np.tile(np.array([[4, 4]], np.int32), (30, 1)), 3)])[0]
    assert got['info'].tolist() == [fgr_ref.NOTHING, 0, 3000, 0] and np.array_equal(got['T'], np.eye(4))
    # rows on one line, in exact arithmetic (dyadic points on the x axis, centred): the rotation about the line is unobservable,
    # H[0][0] == 0 exactly in any summation order -> FAILED in the first step, the identity, no update, the weights of that step
    line = np.zeros((9, 3), np.float32)
    line[:, 0] = np.arange(-4, 5) / 4.0
    c9 = np.stack([np.arange(9), np.arange(9)], 1).astype(np.int32)
    want = fgr_ref.fgr(line, line, c9, 2)
    got = _call(dev, [(line, line, c9, 2)])[0]
    assert np.array_equal(got['info'], want['info']) and got['info'][0] == fgr_ref.FAILED and got['info'][3] == 0
    assert np.array_equal(got['T'], np.eye(4)) and np.array_equal(got['rows'], want['rows'])
    assert np.array_equal(got['weights'], want['weights'], equal_nan=True)
    # a line in general position: FAILED or OK exactly as the restatement decides, and where it is OK the same pose
    rng = np.random.default_rng(4)
    gen = (rng.random(3) + np.outer(np.linspace(0, 1, 40), rng.normal(size=3))).astype(np.float32)
    c40 = np.stack([np.arange(40), np.arange(40)], 1).astype(np.int32)
    want = fgr_ref.fgr(gen, gen, c40, 2)
    got = _call(dev, [(gen, gen, c40, 2)])[0]
    print(f'FGR general line: info {got["info"].tolist()} (ref {want["info"].tolist()}), max |dT| = {np.abs(got["T"] - want["T"]).max():.3e}')
    assert np.array_equal(got['info'], want['info'])
    # clouds of one repeated point: D == 0
    one = np.tile(src[:1], (50, 1))
    got = _call(dev, [(one, one, c40, 2)])[0]
    assert got['info'].tolist() == [fgr_ref.NOTHING, 0, 4000, 0] and np.array_equal(got['T'], np.eye(4)) and np.isnan(got['weights']).all()


def test_batch_independence(dev):
    a, b = _pair(41, 300), _pair(42, 1500)
    five = _pair(43, 40, 5, false_frac=0.0)
    empty = (a[0][:7], a[1][:9], np.zeros((0, 2), np.int32))
    pairs = [empty + (0,), five + (1,), a + (2,), b + (3,)]
    batch = _call(dev, pairs)
    assert batch[0]['info'].tolist() == [fgr_ref.NOTHING, 0, 0, 0] and np.array_equal(batch[0]['T'], np.eye(4))
    assert batch[1]['info'][2] == 500 and 0 < batch[1]['info'][1] < 500      # five correspondences, drawn with replacement
    assert batch[2]['info'].tolist()[:2] == [fgr_ref.OK, 1000] and batch[3]['info'].tolist()[:2] == [fgr_ref.OK, 1000]
    for k, p in enumerate(pairs):
        assert _same(_call(dev, [p])[0], batch[k]), f'pair {k} differs alone'
    rev = _call(dev, pairs[::-1])[::-1]
    again = _call(dev, pairs)
    for k in range(4):
        assert _same(rev[k], batch[k]), f'pair {k} differs in the reversed batch'
        assert _same(again[k], batch[k]), f'pair {k} differs on a rerun'
    # without rows_out / weights_out (the list then lives in the workspace): the same poses and bookkeeping
    bare = _call(dev, pairs, want_rows=False)
    for k in range(4):
        assert np.array_equal(bare[k]['T'], batch[k]['T']) and np.array_equal(bare[k]['info'], batch[k]['info'])


@pytest.mark.parametrize('case', range(4))
def test_robustness(dev, case):
    """half (the variant: two thirds) of the rows are false; defaults, seed 11 + case"""
    for variant in (False, True):
        src, tgt, corr, T, seed = fgr_cases.robust_case(case, variant)
        got = _call(dev, [(src, tgt, corr, seed)])[0]
        rre, rte = fgr_cases.errors(got['T'], T)
        plain = fgr_cases.errors(fgr_cases.kabsch64(src[corr[:, 0]], tgt[corr[:, 1]]), T)
        print(f'FGR robustness case {case} variant {variant}: info {got["info"].tolist()}, {rre:.3e} deg, {rte:.3e}; plain Kabsch over all '
              f'rows {plain[0]:.2f} deg, {plain[1]:.3f}')
        assert got['info'][0] == fgr_ref.OK and got['info'][1] == 1000 and got['info'][3] == 64
        assert rre <= 0.5 and rte <= 0.01
        if not variant:
            assert plain[0] > 5.0                                # the case cannot pass without the line process


BAD = [dict(tuple_scale=0.0), dict(tuple_scale=1.0001), dict(tuple_scale=float('nan')), dict(max_tuples=0), dict(max_tuples=4097),
       dict(trial_factor=0), dict(trial_factor=1 << 30), dict(mu_start=0.0), dict(mu_start=float('inf')), dict(delta=0.0),
       dict(delta=float('nan')), dict(division_factor=1.0), dict(division_factor=float('inf')), dict(division_factor=-2.0),
       dict(decrease_every=0), dict(iterations=-1)]


def test_error_codes(dev):
    L = _lib()
    p = _pair(41, 300) + (2,)
    for opts in BAD:
        raw = _raw_call(dev, [p], opts, expect=BUF_EINVAL)
        assert _untouched(raw), opts
    for null in ('sl', 'tl', 'cl', 'seeds', 'T', 'info', 'ws', 'src', 'tgt', 'corr'):
        assert _untouched(_raw_call(dev, [p], {}, expect=BUF_EINVAL, null=(null,))), null
    assert _untouched(_raw_call(dev, [p], {}, expect=BUF_EINVAL, ws_short=1))
    neg = np.array([-1], np.int32)
    one = np.array([1], np.int32)
    seeds = np.array([0], np.uint64)
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    for lens in ((neg, one, one), (one, neg, one), (one, one, neg)):
        rc = L.buf_fgr_batched(_p(buf), hp(lens[0]), _p(buf), hp(lens[1]), _p(buf), hp(lens[2]), 1, hp(seeds), 0.95, 10, 100, 1.0, 0.025, 0,
                               1.4, 4, 64, _p(buf), _p(buf), None, None, _p(buf), 4096 * 8, _stream())
        assert rc == BUF_EINVAL
    assert L.buf_fgr_batched(None, None, None, None, None, None, -1, None, 0.95, 10, 100, 1.0, 0.025, 0, 1.4, 4, 64, None, None, None,
                             None, None, 0, _stream()) == BUF_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0).all()
    # npairs == 0: accepted with null pointers
    assert L.buf_fgr_batched(None, None, None, None, None, None, 0, None, 0.95, 10, 100, 1.0, 0.025, 0, 1.4, 4, 64, None, None, None,
                             None, None, 0, _stream()) == 0
    assert L.buf_fgr_ws_bytes(100, 0, 10) == 0 and L.buf_fgr_ws_bytes(100, 2, 10) > 0


def test_ops_layer(dev):
    """ops.fgr_batched and fgr.fast_global_registration return what the C entry point writes"""
    from buffer_amd import fgr, ops
    pairs = [_pair(41, 300) + (2,), _pair(42, 1500) + (3,)]
    want = _call(dev, pairs)
    d = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(p[k], dt) for p in pairs])).to(dev)
    lens = lambda k: [len(p[k]) for p in pairs]
    T, info, rows, wts = ops.fgr_batched(d(0, np.float32), lens(0), d(1, np.float32), lens(1), d(2, np.int32), lens(2), [2, 3], return_rows=True)
    res = fgr.fast_global_registration(d(0, np.float32), lens(0), d(1, np.float32), lens(1), d(2, np.int32), lens(2), seeds=[2, 3])
    assert sorted(res) == ['iterations', 'poses', 'status', 'trials', 'tuples'] and res['poses'].dtype == torch.float64
    for b in range(2):
        assert np.array_equal(T[b].cpu().numpy(), want[b]['T']) and np.array_equal(info[b].cpu().numpy(), want[b]['info'])
        assert np.array_equal(rows[b].cpu().numpy(), want[b]['rows']) and np.array_equal(wts[b].cpu().numpy(), want[b]['weights'], equal_nan=True)
        assert np.array_equal(res['poses'][b].cpu().numpy(), want[b]['T']) and int(res['iterations'][b]) == 64
        assert ops.FGR_STATUS[int(res['status'][b])] == 'OK' and int(res['tuples'][b]) == 1000
    with pytest.raises(ValueError):
        ops.fgr_batched(d(0, np.float32), lens(0), d(1, np.float32), lens(1), d(2, np.int32), [1, 2], [2, 3])
    with pytest.raises(ValueError):
        ops.fgr_batched(d(0, np.float32), lens(0), d(1, np.float32), lens(1), d(2, np.int32), lens(2), [2])
    # decrease_mu=False: a floor that mu never passes, so mu stays at mu_start -- the bits of the C call with that floor, not the annealed ones
    fixed = fgr.fast_global_registration(d(0, np.float32), lens(0), d(1, np.float32), lens(1), d(2, np.int32), lens(2), seeds=[2, 3],
                                         decrease_mu=False, return_rows=True)
    flat = _call(dev, pairs, delta=1.7976931348623157e308)
    for b in range(2):
        assert np.array_equal(fixed['poses'][b].cpu().numpy(), flat[b]['T'])
        assert np.array_equal(fixed['weights'][b].cpu().numpy(), flat[b]['weights'], equal_nan=True)
        assert np.nanmin(flat[b]['weights']) > np.nanmin(want[b]['weights'])        # mu = 1 forgives what the annealed mu does not
