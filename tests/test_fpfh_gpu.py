"""buf_fpfh (csrc/fpfh.hip: k_spfh, k_fpfh) through its C entry point against the float64 restatement tests/fpfh_ref.py (pinned by
tests/test_fpfh_cpu.py), on the neighbour rows the device grid gives.

Inputs are seeded uniform points in the unit cube with fp32-rounded unit normals.  Every case first asserts, on the CPU, that the
restatement's margin (smallest distance of an unclamped bin coordinate to an integer) is >= 1e-9: the kernel's fp64 atan2 is a few
ulp from libm's, so with that margin every bin decision is the same and
    spfh_out equals the restatement EXACTLY;
    fpfh_out: the kernel and the restatement run the same fp64 operations in the same order on that table (weights 1 / d2, the
    sum over the columns, the block sums), so it is compared exactly as well -- measured on an MI355X: max |difference| = 0 in
    every case of this file (each case prints its own), and a limit of 2 x that measurement is array_equal.
Outputs are prefilled with NaN and carry a guard past their end.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fpfh_ref

pytestmark = pytest.mark.gpu
BUF_EINVAL = -1
GUARD = 256
MARGIN = 1e-9


def _lib():
    from buffer_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _cloud(seed, n, special=False):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    if special:
        pts[5] = pts[3]                                          # one duplicated point
        nrm[7, 1] = np.nan                                       # one NaN normal
    return pts, nrm


def _rows(dev, pts, radius, k, lengths=None):
    """the device grid's sorted radius rows int32[n,k] (host copy)"""
    from buffer_amd import ops
    t = torch.from_numpy(pts).to(dev)
    lens = np.array([len(pts)] if lengths is None else lengths, np.int32)
    nbr = ops.CellGrid(t, lens, radius).query(t, lens, k)
    torch.cuda.synchronize()
    return nbr.cpu().numpy()


def _call(dev, pts, nrm, nbr, max_nn, with_spfh=True):
    """buf_fpfh into NaN-prefilled outputs -> (fpfh, spfh or None); every value written, the guards untouched"""
    L = _lib()
    n, k = nbr.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tn, tb = d(pts), d(nrm), d(nbr.astype(np.int32))
    out = torch.full((n * 33 + GUARD,), float('nan'), dtype=torch.float64, device=dev)
    sp = torch.full((n * 33 + GUARD,), float('nan'), dtype=torch.float64, device=dev)
    nbytes = int(L.buf_fpfh_ws_bytes(n))
    ws = torch.full((max(nbytes, 8) // 8 + GUARD,), float('nan'), dtype=torch.float64, device=dev)
    rc = L.buf_fpfh(_p(tp), _p(tn), n, _p(tb), k, int(max_nn), _p(out), _p(sp) if with_spfh else None, _p(ws), nbytes, _stream())
    assert rc == 0, L.buf_last_error()
    torch.cuda.synchronize()
    res = []
    for buf in ((out, sp) if with_spfh else (out, ws)):
        h = buf.cpu().numpy()
        assert np.isnan(h[n * 33:n * 33 + GUARD]).all(), 'write past the end'
        assert not np.isnan(h[:n * 33]).any(), 'a value was not written'
        res.append(h[:n * 33].reshape(n, 33).copy())
    if with_spfh:
        assert np.isnan(ws.cpu().numpy()).all(), 'the workspace was written although spfh_out was given'
    return res[0], res[1]


def _check(name, got, want, margin):
    fp, sp = got
    rs, rf = want
    assert margin >= MARGIN, f'{name}: margin {margin:.3g} -- a wrong input, not a tolerance'
    diff = float(np.abs(fp - rf).max()) if fp.size else 0.0
    print(f'FPFH {name}: margin {margin:.3g}, spfh equal {np.array_equal(sp, rs)}, max |fpfh - ref| = {diff:.3g} (scale 200)')
    assert np.array_equal(sp, rs), f'{name}: spfh differs in {int((sp != rs).sum())} values'
    assert np.array_equal(fp, rf), f'{name}: fpfh differs by {diff:.3g}'


# (name, n, radius, max_nn, seed, special)
CASES = [('n64_isolated', 64, 0.3, 100, 2, False), ('n130', 130, 0.3, 100, 1, False), ('n257', 257, 0.3, 100, 0, False),
         ('n257_max8', 257, 0.3, 8, 0, False), ('n300_long', 300, 0.45, 128, 3, False), ('n257_dup_nan', 257, 0.3, 100, 0, True)]


@pytest.mark.parametrize('name,n,radius,max_nn,seed,special', CASES, ids=[c[0] for c in CASES])
def test_fpfh_matches_the_restatement(dev, name, n, radius, max_nn, seed, special):
    pts, nrm = _cloud(seed, n, special)
    k = 100 if max_nn < 100 else max_nn                         # max_nn 8 truncates rows queried at 100 columns
    nbr = _rows(dev, pts, radius, k)
    cnt = (nbr < n).sum(1)
    if name == 'n64_isolated':
        assert (cnt == 1).any() and (cnt >= 2).any()            # rows that hold only the point itself
    if name == 'n257':
        assert cnt.max() <= 64 and cnt.max() >= 30
    if name == 'n257_max8':
        assert (cnt > 8).any()
    if name == 'n300_long':                                     # both lane trips, and the grid's long-row pass
        assert (cnt == 63).any() and (cnt == 64).any() and (cnt >= 65).any(), np.bincount(cnt)[60:70]
    rs, rf, margin = fpfh_ref.fpfh(pts, nrm, nbr, max_nn)
    got = _call(dev, pts, nrm, nbr, max_nn)
    _check(name, got, (rs, rf), margin)
    if special:
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    if name == 'n130':                                          # the SPFH table in the workspace: the same bits
        f2, s2 = _call(dev, pts, nrm, nbr, max_nn, with_spfh=False)
        assert np.array_equal(f2, got[0]) and np.array_equal(s2, got[1])


def test_empty_single_and_two_points(dev):
    L = _lib()
    guard = torch.full((GUARD,), float('nan'), dtype=torch.float64, device=dev)
    assert L.buf_fpfh(None, None, 0, None, 4, 100, _p(guard), _p(guard), None, 0, _stream()) == 0          # touches nothing
    assert L.buf_fpfh(None, None, 0, None, 4, 100, None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert np.isnan(guard.cpu().numpy()).all() and L.buf_fpfh_ws_bytes(0) == 0
    one = np.array([[0.25, 0.5, 0.75]], np.float32)
    fp, sp = _call(dev, one, np.array([[0, 0, 1]], np.float32), _rows(dev, one, 0.3, 4), 100)
    assert not fp.any() and not sp.any()
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    nbr = _rows(dev, two, 1.5, 4)
    assert nbr.tolist() == [[0, 1, 2, 2], [1, 0, 2, 2]]
    fp, sp = _call(dev, two, nrm, nbr, 100)
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(sp, np.stack([want, want])) and np.array_equal(fp, 2 * np.stack([want, want]))
    far = _rows(dev, two, 0.5, 4)                               # out of each other's reach: rows of one, zeros
    fp, sp = _call(dev, two, nrm, far, 100)
    assert not fp.any() and not sp.any()


def test_stacked_clouds_give_the_bits_of_single_calls_and_reruns_agree(dev):
    from buffer_amd import fpfh, ops
    (pa, na), (pb, nb_) = _cloud(1, 130), _cloud(0, 257)
    t = lambda a: torch.from_numpy(a).to(dev)
    single = {}
    for key, (p, nr) in (('a', (pa, na)), ('b', (pb, nb_))):
        nbr = _rows(dev, p, 0.3, 100)
        single[key] = _call(dev, p, nr, nbr, 100)
        assert np.array_equal(fpfh.compute_fpfh(t(p), t(nr), 0.3, 100).cpu().numpy(), single[key][0])
    for order in ('ab', 'ba'):
        ps = np.concatenate([pa, pb] if order == 'ab' else [pb, pa])
        ns = np.concatenate([na, nb_] if order == 'ab' else [nb_, na])
        lens = [130, 257] if order == 'ab' else [257, 130]
        nbr = _rows(dev, ps, 0.3, 100, lens)
        assert ((nbr < lens[0])[:lens[0]] | (nbr == 387)[:lens[0]]).all()                 # the rows stay inside a cloud
        fp, sp = _call(dev, ps, ns, nbr, 100)
        fp2, sp2 = _call(dev, ps, ns, nbr, 100)
        assert np.array_equal(fp, fp2) and np.array_equal(sp, sp2)                          # rerun: the same bits
        first, second = (single['a'], single['b']) if order == 'ab' else (single['b'], single['a'])
        assert np.array_equal(fp, np.concatenate([first[0], second[0]])) and np.array_equal(sp, np.concatenate([first[1], second[1]]))
        F = fpfh.compute_fpfh(t(ps), t(ns), 0.3, 100, lens)
        assert np.array_equal(F.cpu().numpy(), fp)
        f2, s2 = ops.fpfh(t(ps), t(ns), t(nbr), 100, return_spfh=True)
        assert np.array_equal(f2.cpu().numpy(), fp) and np.array_equal(s2.cpu().numpy(), sp)


def test_match_agrees_with_its_numpy_twin(dev):
    from buffer_amd import fpfh
    rng = np.random.default_rng(5)
    fa, fb = rng.random((301, 33)) * 100, rng.random((257, 33)) * 100
    fb[:100] = fa[200:300] + rng.normal(scale=0.5, size=(100, 33))                           # planted mutual matches
    t = lambda a: torch.from_numpy(a).to(dev)
    for mutual in (False, True):
        got = fpfh.match(t(fa), t(fb), mutual)
        assert got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), fpfh_ref.match(fa, fb, mutual))
    m = fpfh.match(t(fa), t(fb), True).cpu().numpy()
    assert len(m) >= 100 and {(200 + i, i) for i in range(100)} <= set(map(tuple, m.tolist()))
    assert fpfh.match(t(fa[:0]), t(fb)).shape == (0, 2)


def test_c_abi_error_codes(dev):
    L = _lib()
    pts, nrm = _cloud(0, 257)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tn = d(pts), d(nrm)
    nbr = d(fpfh_ref.radius_rows(pts, 0.2, 16))
    out = torch.full((257 * 33,), float('nan'), dtype=torch.float64, device=dev)
    need = int(L.buf_fpfh_ws_bytes(257))
    assert need >= 257 * 33 * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda n, k, max_nn, o, sp, w, wb: L.buf_fpfh(_p(tp), _p(tn), n, _p(nbr), k, max_nn, o, sp, w, wb, _stream())
    assert call(257, 16, 1, _p(out), _p(out), None, 0) == BUF_EINVAL and b'max_nn' in L.buf_last_error()
    assert call(257, 16, 129, _p(out), _p(out), None, 0) == BUF_EINVAL
    assert call(257, 16, 100, None, _p(out), None, 0) == BUF_EINVAL and b'null output' in L.buf_last_error()
    assert call(257, 16, 100, _p(out), None, _p(ws), need - 1) == BUF_EINVAL and b'workspace' in L.buf_last_error()
    assert call(257, 16, 100, _p(out), None, None, need) == BUF_EINVAL
    assert call(-1, 16, 100, _p(out), _p(out), None, 0) == BUF_EINVAL
    assert call(257, 0, 100, _p(out), _p(out), None, 0) == BUF_EINVAL
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()                   # refused before any device work
    assert call(257, 16, 100, _p(out), None, _p(ws), need) == 0
    torch.cuda.synchronize()
    assert not np.isnan(out.cpu().numpy()).any()
