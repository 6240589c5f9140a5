"""The seven vector-neuron kernels of csrc/vn.hip (k_vn_gather, k_vn_gather6_lds, k_vn_linear_pre, k_vn_gather_pre, k_vn_pointwise,
k_gather_max, k_vn_std), each through its C entry point against the float64 restatement tests/vn_ref.py (pinned by
tests/test_vn_ref_cpu.py), at the sizes where a launch decision, a block remap, a tail or a branch changes.

Every call writes into a buffer prefilled with NaN that carries guard values past its end: all n * 3 * cout values must have been
written and the guard must be untouched, which is what makes a wrong block remap or tail visible.

Tolerance of the kernels with the fp32 activation (gather blocks, buf_vn_pointwise with map_to_dir): errors are normalised by the
tensor scale max|reference|; e_hip is the kernel against vn_ref in float64, e_fp32 the SAME formulas evaluated by vn_ref in float32 on
the same inputs (one fixed summation order, tests/vn_ref.py).  The kernels sum in fp64 and run the activation in fp32, so they should
be no less accurate than that fp32 run: the assertion is e_hip <= R * e_fp32 with R twice the largest ratio measured on an MI355X.
No case is excluded and no element is masked.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vn_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF_EINVAL = -1
GUARD = 512                    # floats past the end of every output
# e_hip / e_fp32 measured on an MI355X over every case of this file (each test prints its own; DESIGN.md section 4 has the table):
#   gather blocks   0.17 ... 1.000: largest 1.000 (m6_k1, m6_nq32, m1_k1: few input channels, where the kernel's fp32 operations ARE the
#                   fp32 run's and e_hip == e_fp32 to the digit); next 0.92 (m6_nq1); K = 47 staged 0.32, K = 48 direct 0.22, K = 96 0.17 / 0.25 / 0.28
#   buf_vn_pointwise 0.05 ... 0.82 on the layer cases (largest: cout40_residual), 1.000 on the hand-built edge rows (two input channels)
# with e_fp32 between 7e-8 and 5.4e-7 of scale (3.3e-6 for the 60-channel fp32 sum of both_stride21).  Each limit is twice its largest ratio.
R_GATHER = 2.0
R_POINTWISE = 2.0


# ----------------------------------------------------------------------------------------------------------------- weights
_W = {}


def _released():
    if 'w' not in _W:
        from buffer_amd.weights import load_weights
        _W['w'] = load_weights("3dmatch")
    return _W['w']


def _layer(spec, cout, cinp, bn=True):
    """(wf, wd, bsc, bsh) as the fp32 arrays the kernel gets.  spec: a released layer's name (widths must match) or a seed."""
    if isinstance(spec, str):
        wf, wd, bsc, bsh = vn_ref.layer(_released(), spec, np.float32)
        assert wf.shape == (cout, cinp), (spec, wf.shape, cout, cinp)
        return np.ascontiguousarray(wf), np.ascontiguousarray(wd), bsc, bsh
    rng = np.random.default_rng(spec)
    wf = (rng.normal(size=(cout, cinp)) / np.sqrt(cinp)).astype(np.float32)
    wd = (rng.normal(size=(cout, cinp)) / np.sqrt(cinp)).astype(np.float32)
    if not bn:
        return wf, wd, None, None
    return wf, wd, rng.uniform(0.5, 2.0, cout).astype(np.float32), rng.normal(scale=0.3, size=cout).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- C ABI
def _lib():
    from buffer_amd import _lib as L
    return L.lib()


def _d(a, dev, dtype=torch.float32):
    """numpy -> device tensor (None stays None; an empty array gives a tensor whose pointer is null)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype).contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(n_vals, dev):
    return torch.full((n_vals + GUARD,), float('nan'), dtype=torch.float32, device=dev)


def _take(buf, n, width, what):
    """the n x width result; every value written, the guard past the end untouched"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    out, guard = h[:n * width].reshape(n, width), h[n * width:]
    assert not np.isnan(out).any(), f'{what}: {int(np.isnan(out).any(1).sum())} of {n} rows not (fully) written'
    assert np.isnan(guard).all(), f'{what}: wrote past the end of the output'
    return out


def _gather(dev, c, form, nq=None):
    """one gather case through the C ABI.  form: 'block' = buf_vn_gather_block (mode 6: staged or direct as the launcher decides;
    mode 1: the direct kernel), 'pre' = buf_vn_gather_block_pre.  nq: the first nq queries only (default: all)."""
    L = _lib()
    nq = c['nq'] if nq is None else nq
    wf, wd, bsc, bsh = c['layer']
    t = [_d(c[k], dev) for k in ('q', 's', 'feats')] + [_d(c['idx'], dev, torch.int32)] + [_d(x, dev) for x in (wf, wd, bsc, bsh)]
    buf = _out(nq * 3 * c['cout'], dev)
    if form == 'block':
        rc = L.buf_vn_gather_block(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), nq, c['ns'], c['k'], c['cin'], c['cout'], c['mode'],
                                   c['scale'], _p(t[4]), _p(t[5]), _p(t[6]), _p(t[7]), c['slope'], _p(buf), _stream())
    else:
        wsb = L.buf_vn_gather_pre_ws_bytes(c['ns'], c['cout'])
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = L.buf_vn_gather_block_pre(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), nq, c['ns'], c['k'], c['cin'], c['cout'], c['scale'],
                                       _p(t[4]), _p(t[5]), _p(t[6]), _p(t[7]), c['slope'], _p(buf), _p(ws), wsb, _stream())
    assert rc == 0, L.buf_last_error()
    return _take(buf, nq, 3 * c['cout'], f"{c['name']} ({form})")


def _pointwise(dev, a, ind_a, ind_stride, b, n, cout, wf, wd, bsc, bsh, slope, residual, what):
    L = _lib()
    na, ca = (a.shape[0], a.shape[1] // 3) if a is not None else (0, 0)
    cb = b.shape[1] // 3 if b is not None else 0
    t = [_d(a, dev), _d(ind_a, dev, torch.int32), _d(b, dev)] + [_d(x, dev) for x in (wf, wd, bsc, bsh, residual)]
    buf = _out(n * 3 * cout, dev)
    rc = L.buf_vn_pointwise(_p(t[0]), _p(t[1]), ind_stride, na, ca, _p(t[2]), cb, n, cout, _p(t[3]), _p(t[4]), _p(t[5]), _p(t[6]),
                            slope, _p(t[7]), _p(buf), _stream())
    assert rc == 0, L.buf_last_error()
    return _take(buf, n, 3 * cout, what)


def _errors(got, ref64, ref32, what):
    scale = np.abs(ref64).max()
    e_hip, e_fp32 = np.abs(got - ref64).max() / scale, np.abs(ref32 - ref64).max() / scale
    print(f'RATIO {what}: e_hip {e_hip:.3e}  e_fp32 {e_fp32:.3e}  ratio {e_hip / e_fp32 if e_fp32 > 0 else np.inf:.3f}  (scale {scale:.3g})')
    return e_hip, e_fp32


# ----------------------------------------------------------------------------------------------------------------- gather cases
# name: (mode, nq, ns, K, cin, cout, scale, weights)     7 * 32 + 5 = 229, 8 * 32 = 256, 9 * 32 + 1 = 289, 13 * 32 + 5 = 421 queries
# K = 47 | 48: mode 6 on the staged | the direct kernel (4 (8 cout + 256 K + 128) bytes <=> 48 KiB at cout = 10); K = 96: the largest
# slot stage of buf_vn_gather_block_pre, and mode 6 on the direct kernel; 47, 48 and 96 each with a partial last workgroup.
# K = 5: the tail of the loop unrolled by four; cout 7: no divisor of 256 or of 32 * cout / 256 rounds.  Every case has at least 90
# output values, so that neither error of the ratio is the luck of a handful of roundings.
GATHER = {
    'm6_nq1':     (6, 1, 150, 16, 1, 40, 1.0, 11),
    'm6_k1':      (6, 229, 150, 1, 1, 10, 1.0, 'Ref.encoder_blocks.0.conv'),
    'm6_nq31':    (6, 31, 150, 3, 1, 1, 1.0, 12),
    'm6_nq32':    (6, 32, 150, 4, 1, 5, 1.0, 13),
    'm6_nq33':    (6, 33, 150, 5, 1, 7, 1.0, 14),
    'm6_scale5':  (6, 229, 300, 16, 1, 10, 5.0, 'Ref.encoder_blocks.0.conv'),
    'm6_half':    (6, 256, 300, 16, 1, 40, 0.5, 15),
    'm6_k47':     (6, 289, 400, 47, 1, 10, 1.0, 'Ref.encoder_blocks.0.conv'),
    'm6_k48':     (6, 289, 400, 48, 1, 10, 1.0, 'Ref.encoder_blocks.0.conv'),
    'm6_k96':     (6, 421, 400, 96, 1, 10, 1.0, 'Ref.encoder_blocks.0.conv'),
    'm6_ns0':     (6, 33, 0, 5, 1, 10, 1.0, 'Ref.encoder_blocks.0.conv'),
    'm6_outdoor': (6, 229, 300, 16, 1, 10, 1.0, 'Ref.encoder_blocks.0.conv'),
    'm1_nq1':     (1, 1, 150, 16, 40, 40, 1.0, 21),
    'm1_k1':      (1, 229, 150, 1, 1, 1, 1.0, 22),
    'm1_nq31':    (1, 31, 150, 3, 3, 7, 1.0, 23),
    'm1_nq32':    (1, 32, 150, 4, 10, 5, 1.0, 'Ref.encoder_blocks.1.conv'),
    'm1_nq33':    (1, 33, 150, 5, 10, 10, 1.0, 'Ref.encoder_blocks.2.conv'),
    'm1_scale5':  (1, 229, 300, 16, 40, 40, 5.0, 24),
    'm1_half':    (1, 256, 300, 16, 10, 5, 0.5, 'Ref.encoder_blocks.1.conv'),
    'm1_k47':     (1, 289, 400, 47, 3, 10, 1.0, 25),
    'm1_k48':     (1, 289, 400, 48, 10, 5, 1.0, 'Ref.encoder_blocks.1.conv'),
    'm1_k96':     (1, 421, 400, 96, 10, 10, 1.0, 'Ref.encoder_blocks.2.conv'),
    'm1_ns0':     (1, 33, 0, 5, 10, 5, 1.0, 'Ref.encoder_blocks.1.conv'),
    'm1_outdoor': (1, 229, 300, 16, 10, 5, 1.0, 'Ref.encoder_blocks.1.conv'),
    'm1_k97':     (1, 45, 150, 97, 10, 5, 1.0, 'Ref.encoder_blocks.1.conv'),      # past the slot stage of _pre (section "K > 96")
}
MODE6 = [n for n, c in GATHER.items() if c[0] == 6]
MODE1 = [n for n, c in GATHER.items() if c[0] == 1 and n != 'm1_k97']
EXTRA = 37                     # queries appended for "the same queries as part of a larger call"
_CASES = {}


def _case(name):
    """inputs of a gather case (fp32, built once) with EXTRA more queries than the case uses, and its references (computed once)"""
    if name in _CASES:
        return _CASES[name]
    mode, nq, ns, k, cin, cout, scale, wspec = GATHER[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    outdoor = name.endswith('outdoor')
    nt = nq + EXTRA
    s = rng.uniform(-0.25, 0.25, (ns, 3)) * (4.0 if outdoor else 1.0)
    q = (s[rng.integers(0, ns, nt)] if ns else np.zeros((nt, 3))) + rng.normal(scale=0.02, size=(nt, 3))
    if outdoor:                                                   # coordinates of 80 m, features near 1e-3
        s, q = s + np.array([80.0, -62.0, 3.0]), q + np.array([80.0, -62.0, 3.0])
    feats = rng.normal(size=(ns, 3 * cin)) * (1e-3 if outdoor else 1.0)
    if mode == 6 and not outdoor and ns:
        feats /= np.linalg.norm(feats, axis=1, keepdims=True)     # block 0 reads unit normals
    idx = rng.integers(0, max(ns, 1), (nt, k))
    shadow = rng.random((nt, k)) < 0.2                            # ~20 % shadows, values ns and ns + 5
    idx[shadow] = np.where(rng.random(int(shadow.sum())) < 0.5, ns, ns + 5)
    zero_rows = []
    if nq >= 5:
        idx[1] = ns + 5 * (np.arange(k) % 2)                      # an all-shadow row
        idx[2] = rng.integers(0, max(ns, 1), k)                   # a row without a shadow
        idx[3, 0], idx[4, k - 1] = ns, ns + 5                     # a shadow in slot 0, in slot K - 1
        zero_rows = [1]
    if ns == 0:
        idx = rng.integers(0, 6, (nt, k))                         # every slot a shadow: 0 .. 5 >= ns
        zero_rows = list(range(nq))
    c = dict(name=name, mode=mode, nq=nq, ns=ns, k=k, cin=cin, cout=cout, scale=float(scale), slope=0.2,
             q=q.astype(np.float32), s=s.astype(np.float32).reshape(ns, 3), feats=feats.astype(np.float32).reshape(ns, 3 * cin),
             idx=idx.astype(np.int32), layer=_layer(wspec, cout, cin + (3 if mode == 6 else 1), bn=cout != 1), zero_rows=zero_rows)
    _CASES[name] = c
    return c


def _refs(c):
    if 'ref64' not in c:
        a = (c['q'][:c['nq']], c['s'], c['feats'], c['idx'][:c['nq']]) + c['layer'] + (c['slope'], c['mode'], c['scale'])
        c['ref64'] = vn_ref.gather_block(*a)
        c['ref32'] = vn_ref.gather_block(*a, dtype=np.float32)
        assert c['ref32'].dtype == np.float32
    return c['ref64'], c['ref32']


def _check_gather(c, got, what):
    ref64, ref32 = _refs(c)
    assert got.shape == ref64.shape
    for r in c['zero_rows']:
        assert np.array_equal(got[r], np.zeros_like(got[r])), f'{what}: all-shadow row {r} is not exactly 0'
    if c['ns'] == 0:
        assert not ref64.any()
        return
    e_hip, e_fp32 = _errors(got, ref64, ref32, what)
    # R_GATHER = 2 x the largest ratio measured, 1.000 (the table at the top of this file)
    assert e_hip <= R_GATHER * e_fp32, (what, e_hip, e_fp32)


def run_mode6_cases(path, dev=None):
    """every mode-6 case through buf_vn_gather_block -> .npz.  The child process of the `direct6` fixture runs this with
    BUF_VN_GATHER_DIRECT set (the C side reads the switch once), the tests run the same cases in-process without it."""
    dev = dev or torch.device('cuda:0')
    np.savez(path, **{n: _gather(dev, _case(n), 'block') for n in MODE6})


@pytest.fixture(scope="module")
def direct6(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('vn') / 'direct6.npz')
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_vn_kernels_gpu as M; M.run_mode6_cases(sys.argv[1])"
            % (ROOT, os.path.join(ROOT, 'tests')))
    r = subprocess.run([sys.executable, '-c', code, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, BUF_VN_GATHER_DIRECT='1'))
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("name", MODE6)
def test_gather_mode6(name, dev, direct6):
    """buf_vn_gather_block mode 6: k_vn_gather6_lds up to K = 47 (at cout = 10), k_vn_gather from K = 48, both against float64 under
    the same bound; bit-identical to the direct kernel in every case, to a rerun, and to the same queries inside a larger call"""
    assert 'BUF_VN_GATHER_DIRECT' not in os.environ, 'this process must run the launcher\'s own choice'
    c = _case(name)
    staged = 4 * (8 * c['cout'] + 256 * c['k'] + 128) <= 48 * 1024
    assert staged == {'m6_k47': True, 'm6_k48': False, 'm6_k96': False}.get(name, True)        # the threshold sits where the cases say
    got = _gather(dev, c, 'block')
    _check_gather(c, got, name + (' staged' if staged else ' direct by size'))
    assert np.array_equal(got.view(np.uint32), direct6[name].view(np.uint32)), 'staged and direct mode 6 differ'
    assert np.array_equal(got.view(np.uint32), _gather(dev, c, 'block').view(np.uint32)), 'a rerun differs'
    more = _gather(dev, c, 'block', c['nq'] + EXTRA)
    assert np.array_equal(got.view(np.uint32), more[:c['nq']].view(np.uint32)), 'the same queries inside a larger call differ'


@pytest.mark.parametrize("name", MODE1)
def test_gather_mode1(name, dev):
    """mode 1 on the direct kernel (buf_vn_gather_block through the C ABI needs no switch) and on the hoisted form
    (buf_vn_gather_block_pre: k_vn_linear_pre + k_vn_gather_pre; K = 96 is its largest slot stage), both against float64; the two
    agree within the 2e-6 of scale that test_ops_gpu states; reruns and a larger call give the same bits"""
    c = _case(name)
    direct, pre = _gather(dev, c, 'block'), _gather(dev, c, 'pre')
    _check_gather(c, direct, name + ' direct')
    _check_gather(c, pre, name + ' hoisted')
    if c['ns']:
        d = np.abs(pre - direct).max() / np.abs(direct).max()
        print(f'{name}: hoisted vs direct, max difference / scale = {d:.2e}')
        assert d < 2e-6                                           # (measured here: at most 1.2e-7)
    for form, got in (('block', direct), ('pre', pre)):
        assert np.array_equal(got.view(np.uint32), _gather(dev, c, form).view(np.uint32)), f'{form}: a rerun differs'
        more = _gather(dev, c, form, c['nq'] + EXTRA)
        assert np.array_equal(got.view(np.uint32), more[:c['nq']].view(np.uint32)), f'{form}: the same queries inside a larger call differ'


# ----------------------------------------------------------------------------------------------------------------- K > 96
class _Layer:
    def __init__(self, dev, wf, wd, bsc, bsh, slope=0.2):
        self.wf, self.wd, self.bsc, self.bsh = (_d(x, dev) for x in (wf, wd, bsc, bsh))
        self.cout, self.cin, self.slope = wf.shape[0], wf.shape[1], slope


def test_gather_pre_supported_flips_between_k96_and_k97():
    L = _lib()
    assert L.buf_vn_gather_pre_supported(96, 10, 5) == 1 and L.buf_vn_gather_pre_supported(97, 10, 5) == 0
    assert L.buf_vn_gather_pre_supported(1, 1, 1) == 1 and L.buf_vn_gather_pre_supported(0, 10, 5) == 0
    # the weight stage: 8 * cout * (cin + 1) bytes against 48 KiB
    assert L.buf_vn_gather_pre_supported(16, 95, 64) == 1 and L.buf_vn_gather_pre_supported(16, 96, 64) == 0


def test_gather_pre_refuses_k97_with_nothing_launched(dev):
    """BUF_EINVAL, and neither the output nor the workspace was touched: the refusal comes before the first launch"""
    L = _lib()
    c = _case('m1_k97')
    wf, wd, bsc, bsh = c['layer']
    t = [_d(c[k], dev) for k in ('q', 's', 'feats')] + [_d(c['idx'], dev, torch.int32)] + [_d(x, dev) for x in (wf, wd, bsc, bsh)]
    buf = _out(c['nq'] * 3 * c['cout'], dev)
    wsb = L.buf_vn_gather_pre_ws_bytes(c['ns'], c['cout'])
    ws = torch.full((wsb // 4,), float('nan'), dtype=torch.float32, device=dev)
    rc = L.buf_vn_gather_block_pre(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), c['nq'], c['ns'], c['k'], c['cin'], c['cout'], c['scale'],
                                   _p(t[4]), _p(t[5]), _p(t[6]), _p(t[7]), c['slope'], _p(buf), _p(ws), wsb, _stream())
    torch.cuda.synchronize()
    assert rc == BUF_EINVAL and b'k=97' in L.buf_last_error()
    assert torch.isnan(buf).all().item() and torch.isnan(ws).all().item()


def test_ops_gather_mode1_at_k97_runs_the_direct_kernel(dev):
    """ops.vn_gather_block, mode 1, a neighbour limit past the slot stage of the hoisted form: the right answer instead of an error"""
    from buffer_amd import ops
    assert not os.environ.get('BUF_VN_GATHER_DIRECT')
    c = _case('m1_k97')
    n = c['nq']
    out = ops.vn_gather_block(_Layer(dev, *c['layer']), _d(c['q'][:n], dev), _d(c['s'], dev), _d(c['feats'], dev),
                              _d(c['idx'][:n], dev, torch.int32), 1, c['scale'])
    _check_gather(c, out.cpu().numpy(), 'm1_k97 through ops.vn_gather_block')
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _gather(dev, c, 'block').view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------- buf_vn_pointwise
# name: (n, ca, cb, cout, index stride (0: none), weights, batch-norm, slope, residual)
# n * cout on both sides of 256: 25 * 10 = 250 | 26 * 10 = 260; 1 * 40 | 257 * 1; 85 * 3 = 255 | 86 * 3 = 258
POINTWISE = {
    'b_only_vn1':      (257, 0, 10, 10, 0, 'Ref.inv_layer.0.vn1', True, 0.0, False),
    'b_only_250':      (25, 0, 10, 10, 0, 'Ref.inv_layer.0.vn1', True, 0.0, False),
    'b_only_260':      (26, 0, 10, 10, 0, 'Ref.encoder_blocks.1.unary_shortcut', True, 0.2, False),
    'a_only_identity': (85, 5, 0, 3, 0, 31, True, 0.2, False),
    'a_only_stride1':  (86, 5, 0, 3, 1, 32, True, 0.2, False),
    'both_stride21':   (257, 40, 20, 20, 21, 'Ref.decoder_blocks.1.mlp', True, 0.2, False),
    'both_dec3':       (26, 20, 10, 10, 21, 'Ref.decoder_blocks.3.mlp', True, 0.2, False),
    'both_residual':   (25, 20, 10, 10, 1, 'Keypt.decoder_blocks.3.mlp', True, 0.2, True),
    'cout40_residual': (257, 0, 20, 40, 0, 'Ref.encoder_blocks.4.unary', True, 0.2, True),
    'cout40_n1':       (1, 0, 20, 40, 0, 'Ref.encoder_blocks.4.unary_shortcut', True, 0.2, False),
    'cout1_no_bn':     (257, 0, 5, 1, 0, 'Ref.fc_layer.1', False, 0.2, False),
    'cout1_slope0':    (257, 3, 2, 1, 1, 33, False, 0.0, True),
}


def _pointwise_inputs(name):
    n, ca, cb, cout, stride, wspec, bn, slope, res = POINTWISE[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    na = 40
    a = rng.normal(size=(n if not stride else na, 3 * ca)).astype(np.float32) if ca else None
    b = rng.normal(size=(n, 3 * cb)).astype(np.float32) if cb else None
    ind = None
    if stride:
        ind = rng.integers(0, na, (n, stride)).astype(np.int32)
        ind[:, 1:] = na + 1000                                    # only column 0 may be read (a read of another column shows as zeros)
        ind[rng.random(n) < 0.2, 0] = na                          # closest-pool shadows: indices na and above read as zeros
        ind[0, 0] = na + 5                                        # (with cb > 0: a row whose `a` part is a shadow)
    wf, wd, bsc, bsh = _layer(wspec, cout, ca + cb, bn)
    residual = rng.normal(size=(n, 3 * cout)).astype(np.float32) if res else None
    return n, cout, stride, a, ind, b, wf, wd, bsc, bsh, slope, residual


@pytest.mark.parametrize("name", list(POINTWISE))
def test_pointwise_with_activation(name, dev):
    """buf_vn_pointwise with map_to_dir: a only / b only / both, index stride 1 and 21 with shadow indices, with and without
    batch-norm and residual, slope 0 and 0.2, n * cout on both sides of 256, against float64"""
    n, cout, stride, a, ind, b, wf, wd, bsc, bsh, slope, residual = _pointwise_inputs(name)
    got = _pointwise(dev, a, ind, stride, b, n, cout, wf, wd, bsc, bsh, slope, residual, name)
    ia = None if ind is None else ind[:, 0]
    ref64 = vn_ref.pointwise(a, ia, b, wf, wd, bsc, bsh, slope, residual)
    ref32 = vn_ref.pointwise(a, ia, b, wf, wd, bsc, bsh, slope, residual, dtype=np.float32)
    e_hip, e_fp32 = _errors(got, ref64, ref32, 'pointwise ' + name)
    # R_POINTWISE = 2 x the largest ratio measured, 1.000 (test_activation_edges; 0.82 over these cases)
    assert e_hip <= R_POINTWISE * e_fp32, (name, e_hip, e_fp32)
    if ind is not None and b is None and residual is None:
        assert not got[ind[:, 0] >= a.shape[0]].any()             # a shadow row with nothing else: zero in, exactly zero out


@pytest.mark.parametrize("n,cb,cout,spec", [(26, 5, 3, 'Ref.inv_layer.0.vn_lin.weight'), (1, 20, 40, 41), (257, 5, 1, 42),
                                            (25, 10, 10, 43)])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("indexed", [False, True])
def test_pointwise_plain_linear_is_an_fp64_sum_rounded_once(n, cb, cout, spec, with_residual, indexed, dev):
    """wd null (VNStdFeature.vn_lin): no batch-norm, no activation, with and without residual; indexed: half of the channels come
    through a strided index with shadows.

    Derived bound.  The kernel forms the <= 40 products exactly in fp64 (24 + 24 bits), sums them in fp64 (relative error of the
    sum ~ cin * 2^-53 of sum|terms|, far below fp32 resolution) and rounds ONCE to fp32: the result p is float32(exact) or, where
    the fp64 error crosses a rounding boundary, its neighbour -- within 1 ulp of float32(vn_ref).  With a residual r the kernel adds
    in fp32, out = fl(p + r): the half ulp of p that the first rounding left stays in the sum as an ABSOLUTE error, so the second
    rounding makes it at most 2 ulp where an ulp is taken at the larger of |p| and |p + r| (the same as the ulp of the result
    wherever p and r do not cancel, which is what 'within 2 ulp' can mean for a two-step fp32 sum).  Measured on an MI355X: 0 ulp
    without and 1 ulp with a residual in all 16 cases; the limits stay the derived 1 and 2."""
    rng = np.random.default_rng(1000 * n + cout)
    wf = np.ascontiguousarray(_released()[spec]) if isinstance(spec, str) else rng.normal(size=(cout, cb)).astype(np.float32)
    assert wf.shape == (cout, cb)
    x = rng.normal(size=(n, 3 * cb)).astype(np.float32)
    residual = rng.normal(size=(n, 3 * cout)).astype(np.float32) if with_residual else None
    a = ind = None
    b, stride = x, 0
    if indexed:
        ca = cb // 2
        a, b, stride = rng.normal(size=(30, 3 * ca)).astype(np.float32), np.ascontiguousarray(x[:, :3 * (cb - ca)]), 21
        ind = rng.integers(0, 36, (n, 21)).astype(np.int32)       # 30 .. 35: shadows
    got = _pointwise(dev, a, ind, stride, b, n, cout, wf, None, None, None, 0.2, residual, 'plain linear')
    ia = None if ind is None else ind[:, 0]
    p = vn_ref.pointwise(a, ia, b, wf, None, None, None, 0.2, None)
    ref = p if residual is None else p + residual.astype(np.float64)
    unit = np.spacing(np.maximum(np.abs(p.astype(np.float32)), np.abs(ref.astype(np.float32))))
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) / unit
    print(f'plain linear n={n} cout={cout} residual={with_residual} indexed={indexed}: max {ulps.max():.2f} ulp')
    assert ulps.max() <= (2 if with_residual else 1)


def test_activation_edges(dev):
    """Hand-built (p, d) rows through buf_vn_pointwise.  Two input channels and the selector weights wf = [1 0], wd = [0 1] make p the
    first and d the second input vector (with ONE input channel p and d are multiples of the same vector and cannot be orthogonal),
    one output channel, with and without batch-norm; the rows sit among random ones, which set the tensor scale of the bound.
      p . d = 0 exactly (small integers): the `dot >= 0` side;  d = 0;  p = 0 (under batch-norm: norm = 1e-6, output 0 and finite);
      p = d = 0;  dot = +-2^-20 and +-1e-3: the function is continuous at 0, so the float64 bound holds on both sides."""
    rng = np.random.default_rng(5)
    t = 2.0 ** -20
    edges = [((1, 2, 0), (2, -1, 0)), ((3, 0, -4), (4, 5, 3)), ((1, 2, 3), (0, 0, 0)), ((0, 0, 0), (1, 1, 1)), ((0, 0, 0), (0, 0, 0)),
             ((1, 2, t), (2, -1, 1)), ((1, 2, t), (2, -1, -1)), ((1, 2, 1e-3), (2, -1, 1)), ((1, 2, 1e-3), (2, -1, -1)),
             ((1, 2, 0), (-2, 1, 0)), ((1, 2, 2), (-1, -2, -2))]
    x = rng.normal(size=(300, 6)).astype(np.float32)
    x[:len(edges)] = np.array([p + d for p, d in edges], np.float32)
    assert all(np.dot(np.float32(p), np.float32(d)) == 0 for p, d in edges[:2])
    wf, wd = np.array([[1, 0]], np.float32), np.array([[0, 1]], np.float32)
    for bsc, bsh, slope in ((None, None, 0.2), (np.array([1.5], np.float32), np.array([-0.25], np.float32), 0.2),
                            (np.array([0.75], np.float32), np.array([0.5], np.float32), 0.0)):
        what = f'edges bn={bsc is not None} slope={slope}'
        got = _pointwise(dev, None, None, 0, x, 300, 1, wf, wd, bsc, bsh, slope, None, what)
        ref64 = vn_ref.pointwise(None, None, x, wf, wd, bsc, bsh, slope, None)
        ref32 = vn_ref.pointwise(None, None, x, wf, wd, bsc, bsh, slope, None, dtype=np.float32)
        assert np.isfinite(got).all()
        assert not got[3].any() and not got[4].any()              # p = 0: exactly 0, with and without batch-norm
        e_hip, e_fp32 = _errors(got, ref64, ref32, what)
        assert e_hip <= R_POINTWISE * e_fp32, (what, e_hip, e_fp32)           # measured: ratio 1.000 in all three settings


# ----------------------------------------------------------------------------------------------------------------- buf_gather_max
@pytest.mark.parametrize("nq,width,k", [(8, 30, 16), (9, 30, 16), (257, 1, 1), (255, 1, 16), (33, 60, 16), (33, 120, 16), (2, 120, 1),
                                        (3, 120, 16), (5, 60, 1)])
@pytest.mark.parametrize("sign", ["negative", "mixed"])
def test_gather_max_is_exact(nq, width, k, sign, dev):
    """A max of fp32 values is exact: bit-equal to numpy.  All-negative features make the zero shadow row decide: a row with one
    shadow gives 0, a row without gives a negative value, an all-shadow row gives 0.  nq * width on both sides of 256 (8 | 9 x 30,
    255 | 257 x 1, 2 | 3 x 120).  Inputs are finite; what a NaN feature gives is not part of the contract."""
    L = _lib()
    ns = 50
    rng = np.random.default_rng(nq * 1000 + width + k)
    feats = rng.normal(size=(ns, width)).astype(np.float32)
    if sign == "negative":
        feats = -np.abs(feats) - np.float32(0.125)
    idx = rng.integers(0, ns, (nq, k)).astype(np.int32)
    idx[rng.random((nq, k)) < 0.2] = ns
    idx[0] = ns + 5 * (np.arange(k) % 2)                           # all shadow
    idx[1] = rng.integers(0, ns, k)                                # no shadow
    if nq > 2 and k > 1:
        idx[2] = rng.integers(0, ns, k)
        idx[2, k - 1] = ns + 5                                     # one shadow
    t = [_d(feats, dev), _d(idx, dev, torch.int32)]
    buf = _out(nq * width, dev)
    assert L.buf_gather_max(_p(t[0]), _p(t[1]), nq, ns, k, width, _p(buf), _stream()) == 0, L.buf_last_error()
    got = _take(buf, nq, width, 'gather_max')
    want = vn_ref.gather_max(feats, idx, dtype=np.float32)
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[0].any()
    if sign == "negative":
        assert (got[1] < 0).all()
        if nq > 2 and k > 1:
            assert not got[2].any()


# ----------------------------------------------------------------------------------------------------------------- buf_vn_std
@pytest.mark.parametrize("c", [1, 10])
@pytest.mark.parametrize("n", [1, 85, 86])
def test_vn_std_three_term_dot_product(n, c, dev):
    """out[i, 3c + k] = sum_j x[i, c, j] z[i, k, j]; n * c * 3 on both sides of 256 (85 | 86 rows at c = 1).

    Derived bound.  fl(fl(fl(x0 z0) + fl(x1 z1)) + fl(x2 z2)): every term passes through at most three roundings (its product and two
    sums; fewer where the compiler contracts into fma), each of relative size 2^-24, so |error| <= 3 * 2^-24 * sum|x_j z_j| to first
    order.  Asserted exactly so."""
    L = _lib()
    rng = np.random.default_rng(n * 10 + c)
    x = rng.normal(size=(n, 3 * c)).astype(np.float32)
    z = rng.normal(size=(n, 9)).astype(np.float32)
    x[0, :3] = [1.0, 1.0, -2.0]                                    # a cancelling row: the bound stays sum|x z|, not |sum|
    z[0, :3] = [1.0, 1.0, 1.0]
    t = [_d(x, dev), _d(z, dev)]
    buf = _out(n * 3 * c, dev)
    assert L.buf_vn_std(_p(t[0]), _p(t[1]), n, c, _p(buf), _stream()) == 0, L.buf_last_error()
    got = _take(buf, n, 3 * c, 'vn_std')
    ref = vn_ref.vn_std(x, z)
    mag = vn_ref.vn_std(np.abs(x), np.abs(z))
    err = np.abs(got - ref)
    print(f'vn_std n={n} c={c}: max |error| / (2^-24 sum|x z|) = {(err / (2.0 ** -24 * mag)).max():.3f} (limit 3)')
    assert (err <= 3 * 2.0 ** -24 * mag).all()
    assert got[0, 0] == 0.0
