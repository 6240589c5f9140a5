"""buf_sc2_batched (csrc/sc2.hip) through its C entry point against the float64 restatement tests/sc2_ref.py (pinned by
tests/test_sc2_cpu.py, which also asserts the margin conditions of every input compared exactly here).

Exact stage: the live count, counts_out, seeds_out, hyp_counts_out, inliers_out and all of info are chains of decisions (integer
population counts, IEEE comparisons with margins of at least 1e-9 on these inputs) and are compared with array_equal.
Float stage: conf_out and T.  The kernels sum in fixed shapes of their own (column tiles, lanes and trees) where the restatement sums
in ascending order or leaves it to numpy.  Their limits are twice the largest deviation measured on an MI355X over ALL cases
of this file (each case prints its own figures before it asserts):
    max |conf - conf_ref| = 4.663e-15 (rows3000),  max |T - T_ref| = 1.665e-15 (rows3000)
on unit-scale data: a few ulp, far inside the 1e-9 that would be a finding.  By case, |dconf| / |dT|: n0 .. n3 0 / 0 (no pose), n4
0 / 3.3e-16, n63 0 / 7.8e-16, n64 0 / 4.4e-16, n65 and its three option cases 0 / 6.7e-16, n65_dead_dup (both) 0 / 5.6e-16, n127
0 / 3.3e-16, n128 0 / 3.9e-16, n129 and its three option cases 0 / 1.17e-15, n129_dead_dup (both) 0 / 3.3e-16, n300 and its three option
cases 1.33e-15 / 5.6e-16, n300_dead_dup (both) 1.67e-15 / 3.3e-16.  (Up to 128 rows the kernel's confidence sum is the restatement's
ascending sum, the same bits; beyond, it is four partial sums over column tiles and a tree.)
Outputs are prefilled with NaN / -2 / 7 and carry guard words past their end; the workspace has a guard tail.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fgr_cases
import sc2_cases
import sc2_ref

pytestmark = pytest.mark.gpu
BUF_EINVAL = -1
GUARD = 64
THR = sc2_cases.THR
MEASURED_DCONF = 4.67e-15
MEASURED_DT = 1.67e-15
DEFAULTS = dict(d_thr=THR, inlier_thr=THR, **sc2_ref.DEFAULTS)


def _lib():
    from buffer_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


OPTIONAL = ('conf', 'seeds', 'hypc', 'counts', 'inl')


def _raw_call(dev, pairs, opts, detail=True, ws_short=0, expect=0, null=()):
    """pairs: list of (src f32[ns,3], tgt f32[nt,3], corr int[n,2]) -> the raw guarded output buffers after one call"""
    L = _lib()
    o = dict(DEFAULTS, **opts)
    B, ms = len(pairs), int(o['max_seeds'])
    cat = lambda k, w, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(
        [np.asarray(p[k], dt).reshape(-1, w) for p in pairs] + [np.zeros((0, w), dt)]))).to(dev)
    src, tgt, corr = cat(0, 3, np.float32), cat(1, 3, np.float32), cat(2, 2, np.int32)
    sl, tl, cl = (np.array([len(np.asarray(p[k]).reshape(-1, w)) for p in pairs], np.int32) for k, w in ((0, 3), (1, 3), (2, 2)))
    N = int(corr.shape[0])
    msc = ms if 1 <= ms <= 1024 else 1
    full = lambda n, v, dt: torch.full((n + GUARD,), v, dtype=dt, device=dev)
    out = dict(T=full(B * 16, float('nan'), torch.float64), info=full(B * 6, -2, torch.int32), conf=full(N, -2.0, torch.float64),
               seeds=full(B * msc, -2, torch.int32), hypc=full(B * msc, -2, torch.int32), counts=full(msc * N, -2, torch.int32),
               inl=full(N, 7, torch.uint8))
    nbytes = int(L.buf_sc2_ws_bytes(C.c_void_p(cl.ctypes.data), B, ms))
    ws = torch.zeros((max(nbytes, 8) + 8 * GUARD,), dtype=torch.uint8, device=dev)
    ws[nbytes:] = 0xA5
    hp = lambda a: C.c_void_p(a.ctypes.data)
    args = dict(src=_p(src), sl=hp(sl), tgt=_p(tgt), tl=hp(tl), corr=_p(corr), cl=hp(cl), ws=_p(ws), T=_p(out['T']), info=_p(out['info']))
    for k in OPTIONAL:
        args[k] = _p(out[k]) if detail else None
    for k in null:
        args[k] = None
    rc = L.buf_sc2_batched(args['src'], args['sl'], args['tgt'], args['tl'], args['corr'], args['cl'], B, float(o['d_thr']),
                           float(o['inlier_thr']), float(o['seed_ratio']), ms, int(o['k1']), float(o['nms_radius']),
                           int(o['power_iterations']), int(o['refine_iterations']), args['T'], args['info'], args['conf'], args['seeds'],
                           args['hypc'], args['counts'], args['inl'], args['ws'], max(nbytes - ws_short, 0), _stream())
    assert rc == expect, (rc, L.buf_last_error())
    torch.cuda.synchronize()
    assert (ws[nbytes:].cpu().numpy() == 0xA5).all(), 'write past the end of the workspace'
    raw = {k: v.cpu().numpy() for k, v in out.items()}
    raw.update(B=B, ms=msc, N=N, lens=cl)
    return raw


PREFILL = dict(info=-2, conf=-2.0, seeds=-2, hypc=-2, counts=-2, inl=7)
SIZE = dict(T=lambda r: r['B'] * 16, info=lambda r: r['B'] * 6, conf=lambda r: r['N'], seeds=lambda r: r['B'] * r['ms'],
            hypc=lambda r: r['B'] * r['ms'], counts=lambda r: r['ms'] * r['N'], inl=lambda r: r['N'])


def _untouched(raw):
    return bool(np.isnan(raw['T']).all() and all((raw[k] == v).all() for k, v in PREFILL.items()))


def _call(dev, pairs, detail=True, **opts):
    """-> per pair dict(T f64[4,4], info int32[6], conf f64[n], seeds / hyp_counts int32[max_seeds], counts int32[max_seeds,n], inliers
    uint8[n]); every value written, the guards untouched"""
    raw = _raw_call(dev, pairs, opts, detail)
    B, ms = raw['B'], raw['ms']
    assert np.isnan(raw['T'][B * 16:]).all() and not np.isnan(raw['T'][:B * 16]).any()
    for k, v in PREFILL.items():
        m = SIZE[k](raw)
        assert (raw[k][m:] == v).all(), f'{k}: write past the end'
        if detail or k == 'info':
            assert not (raw[k][:m] == v).any(), f'{k}: a value was not written'
        else:
            assert (raw[k] == v).all(), f'{k}: written though null was passed'
    off = np.concatenate([[0], np.cumsum(raw['lens'])])
    res = []
    for b in range(B):
        n, o = int(raw['lens'][b]), int(off[b])
        res.append(dict(T=raw['T'][16 * b:16 * b + 16].reshape(4, 4).copy(), info=raw['info'][6 * b:6 * b + 6].copy(),
                        conf=raw['conf'][o:o + n].copy(), seeds=raw['seeds'][ms * b:ms * (b + 1)].copy(),
                        hyp_counts=raw['hypc'][ms * b:ms * (b + 1)].copy(),
                        counts=raw['counts'][ms * o:ms * (o + n)].reshape(ms, n).copy(), inliers=raw['inl'][o:o + n].copy()))
    return res


KEYS = ('T', 'info', 'conf', 'seeds', 'hyp_counts', 'counts', 'inliers')


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=(k == 'conf')) for k in KEYS)


def _float_stage(label, got, want):
    """prints and returns (max |conf - conf_ref|, max |T - T_ref|); the NaN pattern of conf must be the reference's"""
    assert np.array_equal(np.isnan(got['conf']), np.isnan(want['conf']))
    live = ~np.isnan(want['conf'])
    dc = float(np.abs(got['conf'][live] - want['conf'][live]).max()) if live.any() else 0.0
    dT = float(np.abs(got['T'] - want['T']).max())
    print(f'SC2 {label}: info {got["info"].tolist()} (ref {want["info"].tolist()}), max |dconf| = {dc:.3e}, max |dT| = {dT:.3e}')
    return dc, dT


# ------------------------------------------------------------------------------------------ exact and float stages
@pytest.mark.parametrize('name', [c[0] for c in sc2_cases.EXACT_CASES])
def test_against_the_restatement(dev, name):
    src, tgt, corr, opts, want = sc2_cases.exact_case(name)
    got = _call(dev, [(src, tgt, corr)], **opts)[0]
    dc, dT = _float_stage(name, got, want)
    ms = dict(DEFAULTS, **opts)['max_seeds']
    assert got['info'][1] == want['info'][1]
    assert np.array_equal(got['counts'], want['counts'][:ms]), int((got['counts'] != want['counts'][:ms]).sum())
    assert np.array_equal(got['seeds'], want['seeds'][:ms])
    assert np.array_equal(got['hyp_counts'], want['hyp_counts'][:ms])
    assert np.array_equal(got['inliers'], want['inliers'])
    assert np.array_equal(got['info'], want['info']), (got['info'], want['info'])
    assert dc <= 2 * MEASURED_DCONF and dT <= 2 * MEASURED_DT, (dc, dT)
    n = len(corr)
    if n < 3:
        assert got['info'][0] == sc2_ref.NOTHING and np.array_equal(got['T'], np.eye(4)) and not got['inliers'].any()
    if n >= 63:
        assert got['info'][0] == sc2_ref.OK and got['info'][5] >= 3
    if 'dead_dup' in name:                                       # the dead rows: no confidence, no bit, no seed, no inlier
        dead = [0, 63, 64, n - 1]
        assert np.isnan(got['conf'][dead]).all() and not got['inliers'][dead].any() and not np.isin(dead, got['seeds']).any()
        used = got['counts'][got['seeds'] >= 0]
        assert (used[:, dead] == 0).all() and got['info'][1] == n - len(set(dead))
        assert got['conf'][3] == got['conf'][10] == got['conf'][n - 3]             # the repeated rows tie exactly
    if 'k128' in name and n == 65:
        assert got['info'][0] == sc2_ref.OK                      # k1 above n: the sets are the positive counts


def test_larger_input(dev):
    src, tgt, corr, want = sc2_cases.large_case()
    got = _call(dev, [(src, tgt, corr)])[0]
    dc, dT = _float_stage('rows3000', got, want)
    assert np.array_equal(got['info'], want['info']), (got['info'], want['info'])
    assert np.array_equal(got['seeds'], want['seeds'])
    assert dT <= 2 * MEASURED_DT


# ------------------------------------------------------------------------------------------ robustness
@pytest.mark.parametrize('case', range(4))
def test_robustness(dev, case):
    """half (the variant: two thirds) of the rows are false"""
    for variant in (False, True):
        src, tgt, corr, T, _ = fgr_cases.robust_case(case, variant)
        got = _call(dev, [(src, tgt, corr)])[0]
        rre, rte = fgr_cases.errors(got['T'], T)
        print(f'SC2 robustness case {case} variant {variant}: info {got["info"].tolist()}, {rre:.3e} deg, {rte:.3e}')
        assert got['info'][0] == sc2_ref.OK and rre <= 0.5 and rte <= 0.01


@pytest.mark.parametrize('true_rows', (30, 15))
@pytest.mark.parametrize('case', range(4))
def test_low_inlier_ratio(dev, case, true_rows):
    """10 % and 5 % true rows: the regime where Fast Global Registration and the plain fit are tens of degrees off"""
    src, tgt, corr, T = sc2_cases.low_inlier_case(true_rows, case)
    got = _call(dev, [(src, tgt, corr)])[0]
    rre, rte = fgr_cases.errors(got['T'], T)
    plain = fgr_cases.errors(fgr_cases.kabsch64(src[corr[:, 0]], tgt[corr[:, 1]]), T)
    print(f'SC2 {true_rows} true rows of 300, case {case}: info {got["info"].tolist()}, {rre:.3e} deg, {rte:.3e}; plain Kabsch over all '
          f'rows {plain[0]:.2f} deg, {plain[1]:.3f}')
    assert plain[0] > 5.0                                        # the case cannot pass without the estimator
    assert got['info'][0] == sc2_ref.OK and rre <= 0.5 and rte <= 0.01


# ------------------------------------------------------------------------------------------ batches, errors, layers
def _four_pairs():
    a, b = sc2_cases.exact_case('n300')[:3], sc2_cases.large_case()[:3]
    five = sc2_cases.exact_input(5)
    empty = (a[0][:7], a[1][:9], np.zeros((0, 2), np.int32))
    return [empty, five, a, (b[0], b[1], b[2][:1500])]


def test_batch_independence(dev):
    pairs = _four_pairs()
    batch = _call(dev, pairs)
    assert batch[0]['info'].tolist() == [sc2_ref.NOTHING, 0, 0, -1, 0, 0] and np.array_equal(batch[0]['T'], np.eye(4))
    assert batch[1]['info'][1] == 5 and batch[2]['info'][0] == sc2_ref.OK and batch[3]['info'][0] == sc2_ref.OK
    assert batch[3]['info'][1] == 1500 and batch[3]['info'][5] > 1000
    for k, p in enumerate(pairs):
        assert _same(_call(dev, [p])[0], batch[k]), f'pair {k} differs alone'
    rev = _call(dev, pairs[::-1])[::-1]
    again = _call(dev, pairs)
    for k in range(4):
        assert _same(rev[k], batch[k]), f'pair {k} differs in the reversed batch'
        assert _same(again[k], batch[k]), f'pair {k} differs on a rerun'
    bare = _call(dev, pairs, detail=False)                       # every optional output null
    for k in range(4):
        assert np.array_equal(bare[k]['T'], batch[k]['T']) and np.array_equal(bare[k]['info'], batch[k]['info'])


BAD = [dict(d_thr=0.0), dict(d_thr=float('nan')), dict(d_thr=float('inf')), dict(d_thr=1e200), dict(inlier_thr=0.0), dict(inlier_thr=-1.0),
       dict(inlier_thr=float('inf')), dict(seed_ratio=0.0), dict(seed_ratio=1.5), dict(seed_ratio=float('nan')), dict(max_seeds=0),
       dict(max_seeds=1025), dict(k1=2), dict(k1=129), dict(nms_radius=-0.1), dict(nms_radius=float('nan')), dict(power_iterations=-1),
       dict(refine_iterations=-1)]


def test_error_codes(dev):
    L = _lib()
    p = sc2_cases.exact_case('n300')[:3]
    for opts in BAD:
        assert _untouched(_raw_call(dev, [p], opts, expect=BUF_EINVAL)), opts
    for null in ('sl', 'tl', 'cl', 'T', 'info', 'ws', 'src', 'tgt', 'corr'):
        assert _untouched(_raw_call(dev, [p], {}, expect=BUF_EINVAL, null=(null,))), null
    assert _untouched(_raw_call(dev, [p], {}, expect=BUF_EINVAL, ws_short=1))
    neg, one, big = np.array([-1], np.int32), np.array([1], np.int32), np.array([16385], np.int32)
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    tail = (THR, THR, 0.2, 512, 30, 0.0, 10, 20)
    for lens in ((neg, one, one), (one, neg, one), (one, one, neg), (one, one, big)):
        rc = L.buf_sc2_batched(_p(buf), hp(lens[0]), _p(buf), hp(lens[1]), _p(buf), hp(lens[2]), 1, *tail, _p(buf), _p(buf), None, None,
                               None, None, None, _p(buf), (1 << 16) * 8, _stream())
        assert rc == BUF_EINVAL
    nothing = (None,) * 6
    assert L.buf_sc2_batched(*nothing, -1, *tail, None, None, None, None, None, None, None, None, 0, _stream()) == BUF_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0).all()
    # npairs == 0: accepted with null pointers
    assert L.buf_sc2_batched(*nothing, 0, *tail, None, None, None, None, None, None, None, None, 0, _stream()) == 0
    assert L.buf_sc2_ws_bytes(hp(one), 0, 10) == 0 and L.buf_sc2_ws_bytes(hp(one), 1, 0) == 0 and L.buf_sc2_ws_bytes(hp(big), 1, 10) == 0
    assert L.buf_sc2_ws_bytes(None, 1, 10) == 0 and L.buf_sc2_ws_bytes(hp(one), 1, 10) > 0
    # sized from the actual lengths: the bit matrix and the counts of 300 rows, not of the limit
    assert L.buf_sc2_ws_bytes(hp(np.array([300], np.int32)), 1, 512) < 1 << 20


def test_ops_layer(dev):
    """ops.sc2_batched and sc2.sc2_registration return what the C entry point writes"""
    from buffer_amd import ops, sc2
    pairs = [sc2_cases.exact_case('n300')[:3], sc2_cases.exact_case('n129_dead_dup')[:3]]
    want = _call(dev, pairs)
    d = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(p[k], dt) for p in pairs])).to(dev)
    lens = lambda k: [len(p[k]) for p in pairs]
    args = (d(0, np.float32), lens(0), d(1, np.float32), lens(1), d(2, np.int32), lens(2))
    T, info, det = ops.sc2_batched(*args, THR, THR, return_detail=True)
    res = sc2.sc2_registration(*args, d_thr=THR, return_detail=True)
    plain = sc2.sc2_registration(*args, options=sc2.Sc2Options(d_thr=THR))
    assert sorted(plain) == ['inliers', 'live', 'poses', 'seeds', 'status', 'winner'] and plain['poses'].dtype == torch.float64
    assert ops.sc2_batched(*args, THR, THR)[2] is None
    off = np.concatenate([[0], np.cumsum(lens(2))])
    for b in range(2):
        o, n = int(off[b]), lens(2)[b]
        assert np.array_equal(T[b].cpu().numpy(), want[b]['T']) and np.array_equal(info[b].cpu().numpy(), want[b]['info'])
        assert np.array_equal(det['confidence'][o:o + n].cpu().numpy(), want[b]['conf'], equal_nan=True)
        assert np.array_equal(det['seeds'][b].cpu().numpy(), want[b]['seeds'])
        assert np.array_equal(det['hyp_counts'][b].cpu().numpy(), want[b]['hyp_counts'])
        assert np.array_equal(det['counts'][512 * o:512 * (o + n)].cpu().numpy().reshape(512, n), want[b]['counts'])
        assert np.array_equal(det['inlier_mask'][o:o + n].cpu().numpy(), want[b]['inliers'])
        assert np.array_equal(res['poses'][b].cpu().numpy(), want[b]['T']) and np.array_equal(plain['poses'][b].cpu().numpy(), want[b]['T'])
        assert ops.SC2_STATUS[int(res['status'][b])] == 'OK' and int(res['live'][b]) == want[b]['info'][1]
        assert int(res['seeds'][b]) == want[b]['info'][2] and int(res['winner'][b]) == want[b]['info'][3]
        assert int(res['winner_count'][b]) == want[b]['info'][4] and int(res['inliers'][b]) == want[b]['info'][5]
        assert np.array_equal(res['seed_rows'][b].cpu().numpy(), want[b]['seeds'])
    with pytest.raises(ValueError):
        ops.sc2_batched(args[0], lens(0), args[2], lens(1), args[4], [1, 2], THR, THR)
    with pytest.raises(ValueError):
        ops.sc2_batched(*args, THR, THR, k1=2)
    with pytest.raises(TypeError):
        sc2.sc2_registration(*args, options=sc2.Sc2Options(), d_thr=THR)
