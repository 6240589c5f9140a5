"""buf_feature_match (csrc/match.hip) through the C entry point against the float32 twin of its contract (tests/match_ref.py): every
comparison is EXACT equality -- the twin's float32 operations are the kernel's, correctly rounded and never fused -- so there is no
tolerance anywhere in this file.  Outputs are prefilled with 0xAB bytes and carry a guard past their end; the rows of corr_out past
the total and the guards must come back untouched.  The old path (two ops.knn calls per pair and a mask: fpfh.match) is computed in
the same test where the new rows are compared with it: it is the yardstick, not the new code.
Inputs: match_ref.make_pair, whose counts per filter tests/test_match_cpu.py pins (each filter keeps some matches and drops others)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import match_ref

pytestmark = pytest.mark.gpu
BUF_EINVAL = -1
GUARD = 64                                                        # rows past the end of every output
FILL = 0xAB
FILL_I32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
FILL_U32 = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]


def _lib():
    from buffer_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(dev, pairs, mutual=True, ratio=0.0, with_nn=True, expect=0):
    """buf_feature_match on the stacked pairs into prefilled, guarded outputs -> dict(corr, counts, nn, ssd) (numpy), after checking
    that nothing past the written part changed; expect != 0: the return code only"""
    L = _lib()
    d = pairs[0][0].shape[1]
    al, bl = np.array([len(a) for a, _ in pairs], np.int32), np.array([len(b) for _, b in pairs], np.int32)
    na, nb, P = int(al.sum()), int(bl.sum()), len(pairs)
    up = lambda xs: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs).astype(np.float32).reshape(-1, d))).to(dev)
    fa, fb = up([a for a, _ in pairs]), up([b for _, b in pairs])
    fill = lambda rows, w, dt: torch.full(((rows + GUARD) * w * 4,), FILL, dtype=torch.uint8, device=dev).view(dt).reshape(-1, w)
    corr, counts = fill(na, 2, torch.int32), fill(P, 1, torch.int32)
    nn, sd = (fill(na, 2, torch.int32), fill(na, 2, torch.float32)) if with_nn else (None, None)
    nbytes = L.buf_feature_match_ws_bytes(na, nb, P)
    ws = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    rc = L.buf_feature_match(_p(fa), C.c_void_p(al.ctypes.data), _p(fb), C.c_void_p(bl.ctypes.data), P, d, int(mutual), float(ratio),
                             _p(corr), _p(counts), _p(nn), _p(sd), _p(ws), nbytes, _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, L.buf_last_error())
        for t in (corr, counts) + ((nn, sd) if with_nn else ()):                      # refused before any device work
            assert (t.view(torch.uint8).cpu().numpy() == FILL).all()
        return None
    assert rc == 0, L.buf_last_error()
    assert (ws[nbytes:].cpu().numpy() == FILL).all()
    cn = counts.cpu().numpy().reshape(-1)
    assert (cn[P:] == FILL_I32).all()
    cn = cn[:P].copy()
    m = int(cn.sum())
    co = corr.cpu().numpy()
    assert 0 <= m <= na and (co[m:] == FILL_I32).all()                                # rows past the total and the guard: untouched
    out = dict(corr=co[:m].copy(), counts=cn, nn=None, ssd=None)
    if with_nn:
        nh, sh = nn.cpu().numpy(), sd.cpu().numpy()
        assert (nh[na:] == FILL_I32).all() and (sh[na:].view(np.uint32) == FILL_U32).all()
        out.update(nn=nh[:na].copy(), ssd=sh[:na].copy())
    return out


def _same(got, want, what=''):
    assert np.array_equal(got['counts'], want['counts']), (what, got['counts'], want['counts'])
    assert np.array_equal(got['corr'], want['corr']), what
    if got['nn'] is not None:
        assert np.array_equal(got['nn'], want['nn']), what
        assert np.array_equal(got['ssd'].view(np.uint32), want['ssd'].view(np.uint32)), what      # the bits (and +inf where there is none)


@functools.lru_cache(maxsize=None)
def _pair(case):
    return match_ref.make_pair(*case)


@functools.lru_cache(maxsize=None)
def _want(case, mutual, ratio):
    return match_ref.match_batch([_pair(case)], mutual, ratio)


def _old_path(dev, a, b):
    """the rows the parent's pair-by-pair path gives: two ops.knn calls at k = 1 and the mask (fpfh.match)"""
    from buffer_amd import fpfh
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return fpfh.match(t(a), t(b), True).cpu().numpy()


@pytest.mark.parametrize('case', match_ref.CASES + match_ref.WIDE_CASES, ids=lambda c: 'seed%d-%dx%d-d%d' % c)
def test_cases_against_the_twin(dev, case):
    a, b = _pair(case)
    # on the CPU first: both filters keep some forward matches and drop others on this case
    f, mu, ra = (len(_want(case, m, r)['corr']) for m, r in ((False, None), (True, None), (False, match_ref.RATIO)))
    assert 0 < mu < f and 0 < ra < f
    for mutual, ratio in ((True, None), (False, None), (True, match_ref.RATIO), (False, match_ref.RATIO)):
        got = _call(dev, [(a, b)], mutual, ratio or 0.0)
        _same(got, _want(case, mutual, ratio), (case, mutual, ratio))
    assert np.array_equal(_call(dev, [(a, b)], True, 0.0, with_nn=False)['corr'], _want(case, True, None)['corr'])
    # equivalence to the old path: mutual, no ratio, finite inputs
    assert np.array_equal(_call(dev, [(a, b)], True, 0.0)['corr'], _old_path(dev, a, b))


def test_ratio_values(dev):
    case = match_ref.CASES[0]
    a, b = _pair(case)
    _same(_call(dev, [(a, b)], False, 0.0), _want(case, False, None))                   # 0 switches the test off
    _same(_call(dev, [(a, b)], False, -1.0), _want(case, False, None))
    _same(_call(dev, [(a, b)], False, 0.8), _want(case, False, 0.8))
    _same(_call(dev, [(a, b)], True, 0.5), match_ref.match_batch([(a, b)], True, 0.5))
    for bad in (1.0, 1.5, float('nan'), float('inf')):
        _call(dev, [(a, b)], True, bad, expect=BUF_EINVAL)
        assert b'ratio' in _lib().buf_last_error()


def test_single_reference_row_and_empty_sides(dev):
    a, b = _pair(match_ref.CASES[1])
    one = (a, b[3:4])                                                                   # nb = 1: no second neighbour, the ratio test passes
    for mutual in (True, False):
        want = match_ref.match_batch([one], mutual, match_ref.RATIO)
        _same(_call(dev, [one], mutual, match_ref.RATIO), want)
        assert len(want['corr']) == (1 if mutual else len(a)) and (want['nn'][:, 1] == -1).all()
    # na = 0 and nb = 0 inside a batch, first, in the middle and last
    batch = [(a[:0], b), (a, b), (a[:70], b[:0]), (a[:5], b[:2]), (a[:0], b[:0])]
    for mutual, ratio in ((True, None), (False, match_ref.RATIO)):
        want = match_ref.match_batch(batch, mutual, ratio)
        assert want['counts'][[0, 2, 4]].tolist() == [0, 0, 0] and want['counts'][1] > 0
        _same(_call(dev, batch, mutual, ratio or 0.0), want)
    # no row of A at all: zero counts, nothing else touched; no pairs: nothing touched
    got = _call(dev, [(a[:0], b), (a[:0], b[:0])], True, 0.0)
    assert got['counts'].tolist() == [0, 0] and got['corr'].shape == (0, 2)
    L = _lib()
    cnt = torch.full((GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert L.buf_feature_match(None, None, None, None, 0, 33, 1, 0.0, None, _p(cnt), None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == FILL).all()


def test_duplicated_rows_tie_to_the_lower_index(dev):
    rng = np.random.default_rng(9)
    b = np.repeat(rng.random((70, 33)).astype(np.float32), 2, 0)                        # rows 2k and 2k + 1 are twins
    a = np.repeat(b[rng.permutation(70)[:33] * 2], 2, 0)                                # and so are the queries: every ssd1 == ssd2 == 0
    want = match_ref.match_batch([(a, b)], True, None)
    assert (want['nn'][:, 0] % 2 == 0).all() and (want['nn'][:, 1] == want['nn'][:, 0] + 1).all() and not want['ssd'].any()
    assert (want['corr'][:, 0] % 2 == 0).all() and len(want['corr']) == 33             # the lower twin wins on both sides
    _same(_call(dev, [(a, b)], True, 0.0), want)
    _same(_call(dev, [(a, b)], True, match_ref.RATIO), match_ref.match_batch([(a, b)], True, match_ref.RATIO))     # 0 <= r2 * 0
    assert np.array_equal(_call(dev, [(a, b)], True, 0.0)['corr'], _old_path(dev, a, b))


def test_non_finite_rows(dev):
    a, b = (x.copy() for x in _pair(match_ref.CASES[0]))
    a[3, 5], a[64, 32], a[129, 0] = np.nan, np.inf, -np.inf
    b[int(match_ref.two_nearest(a[:1], b)[0][0, 0]), 7] = np.nan                        # the row a[0] would have matched
    b[100, 0], b[256, 32] = np.inf, np.nan
    bad_b = np.flatnonzero(~np.isfinite(b).all(1))
    for mutual, ratio in ((True, None), (False, None), (True, match_ref.RATIO)):
        want = match_ref.match_batch([(a, b)], mutual, ratio)
        assert (want['nn'][[3, 64, 129]] == -1).all() and not np.isin(want['nn'], bad_b).any() and want['nn'][0, 0] >= 0
        assert not np.isin(want['corr'][:, 0], [3, 64, 129]).any()
        _same(_call(dev, [(a, b)], mutual, ratio or 0.0), want, (mutual, ratio))
    # finite rows whose sum overflows to +inf are ranked like any other
    big = (np.array([[3e38, -3e38] + [0.0] * 31], np.float32), np.array([[-3e38, 3e38] + [0.0] * 31, [3e38, -3e38] + [0.0] * 31], np.float32))
    want = match_ref.match_batch([big], False, 0.5)
    assert want['nn'].tolist() == [[1, 0]] and np.isinf(want['ssd'][0, 1])
    _same(_call(dev, [big], False, 0.5), want)


def test_a_pair_is_the_same_alone_in_a_batch_and_on_a_rerun(dev):
    cases = [c for c in match_ref.CASES if c[3] == 33]                                  # one call has one d
    a0, b0 = _pair(cases[0])
    batch = [_pair(c) for c in cases] + [(a0[:0], b0), (b0, a0), (a0[:63], b0[:1])]
    for mutual, ratio in ((True, None), (True, match_ref.RATIO), (False, match_ref.RATIO)):
        got = _call(dev, batch, mutual, ratio or 0.0)
        _same(got, match_ref.match_batch(batch, mutual, ratio))
        again = _call(dev, batch, mutual, ratio or 0.0)
        for k in ('corr', 'counts', 'nn', 'ssd'):
            assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32))
        co, ro = np.concatenate([[0], np.cumsum(got['counts'])]), np.concatenate([[0], np.cumsum([len(a) for a, _ in batch])])
        for p, pair in enumerate(batch):
            alone = _call(dev, [pair], mutual, ratio or 0.0)
            assert np.array_equal(alone['corr'], got['corr'][co[p]:co[p + 1]])
            assert np.array_equal(alone['nn'], got['nn'][ro[p]:ro[p + 1]])
            assert np.array_equal(alone['ssd'].view(np.uint32), got['ssd'][ro[p]:ro[p + 1]].view(np.uint32))
    # and the old path, pair by pair
    got = _call(dev, batch, True, 0.0)
    co = np.concatenate([[0], np.cumsum(got['counts'])])
    for p, (a, b) in enumerate(batch):
        assert np.array_equal(got['corr'][co[p]:co[p + 1]], _old_path(dev, a, b)), p


def test_argument_errors(dev):
    a, b = _pair(match_ref.CASES[1])
    L = _lib()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fa, fb = t(a), t(b)
    al, bl = np.array([len(a)], np.int32), np.array([len(b)], np.int32)
    hp = lambda x: C.c_void_p(x.ctypes.data)
    corr = torch.full((len(a) * 2,), FILL_I32, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), FILL_I32, dtype=torch.int32, device=dev)
    nbytes = L.buf_feature_match_ws_bytes(len(a), len(b), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ok = [_p(fa), hp(al), _p(fb), hp(bl), 1, 33, 1, 0.0, _p(corr), _p(cnt), None, None, _p(ws), nbytes, _stream()]
    neg = np.array([-1], np.int32)
    for pos, val, word in ((0, None, b'null input'), (1, None, b'null host'), (2, None, b'null input'), (3, None, b'null host'),
                           (1, hp(neg), b'negative length'), (4, -1, b'pairs'), (5, 0, b'd=0'), (5, 65, b'd=65'), (8, None, b'corr_out'),
                           (9, None, b'counts_out'), (12, None, b'workspace'), (13, nbytes - 1, b'workspace')):
        args = list(ok)
        args[pos] = val
        assert L.buf_feature_match(*args) == BUF_EINVAL and word in L.buf_last_error(), (pos, L.buf_last_error())
    torch.cuda.synchronize()
    assert (corr.cpu().numpy() == FILL_I32).all() and (cnt.cpu().numpy() == FILL_I32).all()
    assert L.buf_feature_match(*ok) == 0


def test_python_layers(dev):
    from buffer_amd import fpfh, ops
    cases = [c for c in match_ref.CASES if c[3] == 33]
    batch = [_pair(c) for c in cases]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fa, fb = t(np.concatenate([a for a, _ in batch])), t(np.concatenate([b for _, b in batch]))
    al, bl = [len(a) for a, _ in batch], [len(b) for _, b in batch]
    for mutual, ratio in ((True, None), (False, 0.8)):
        want = match_ref.match_batch(batch, mutual, ratio)
        corr, cl, nn, sd = ops.feature_match(fa.double(), al, fb.double(), bl, mutual=mutual, ratio=ratio, return_nn=True)      # f64 is cast
        assert corr.dtype == torch.int32 and corr.is_cuda and isinstance(cl, np.ndarray) and cl.dtype == np.int32
        assert np.array_equal(corr.cpu().numpy(), want['corr']) and np.array_equal(cl, want['counts'])
        assert np.array_equal(nn.cpu().numpy(), want['nn']) and np.array_equal(sd.cpu().numpy(), want['ssd'])
        assert ops.feature_match(fa, al, fb, bl, mutual=mutual, ratio=ratio)[2:] == (None, None)
        # the stacked src / tgt / src / ... layout of register_batch
        F = t(np.concatenate([x for pair in batch for x in pair])).double()
        c2, l2 = fpfh.match_batch(F, [n for pair in zip(al, bl) for n in pair], mutual, ratio)
        assert torch.equal(c2, corr) and np.array_equal(l2, cl)
    c0, l0, _, _ = ops.feature_match(fa[:0], [], fb[:0], [])
    assert c0.shape == (0, 2) and l0.shape == (0,)
    assert fpfh.match_batch(fa[:0], [])[0].shape == (0, 2)
    for bad in (dict(ratio=1.0), dict(ratio=0.0), dict(ratio=float('nan'))):
        with pytest.raises(ValueError):
            ops.feature_match(fa, al, fb, bl, **bad)
    with pytest.raises(ValueError):
        ops.feature_match(fa, al[:1], fb, bl)
    with pytest.raises(ValueError):
        ops.feature_match(fa, al, fb[:, :32], bl)
    with pytest.raises(ValueError):
        fpfh.match_batch(fa, [len(fa)])                                                  # an odd number of clouds
