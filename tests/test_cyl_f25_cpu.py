"""Host side and code object of the F(2x5) layer forms in the fused kernel k_cyl_net_w25t / k_cyl_net_w25t_rerun (csrc/convnet_w25.hip:
F(2x5, 3x3) tiles -- 2 rows x 5 azimuth
columns, 4 x 4 regular tiles for the 7 x 20 map, 28 matrix instructions per (k-step, N-tile) and no direct round -- in the 64- and
32-output layers of the descriptor CNN): the filter transform against a float64 numpy statement of G2 g G5^T and the transform identity
it rests on, the argument checks of the new entry points, what the two ops classes run with and without f25=, and what the kernels
compiled to, read off the gfx950 code object of the in-tree library.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from test_cyl_code_object_cpu import code_object, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)
from test_cyl_f24_code_object_cpu import KERNELS, beyond, mfma_per_loop
from test_cyl_f24a_cpu import W24A_LOOPS
from test_cyl_f24k_cpu import RELEASED_IN, RELEASED_OUT, ints
from test_winograd_f24_cpu import A2T, B2T, correlate

# MFMAs per k-loop of the body whose newest forms were these (test_matrix_instruction_count says which form accounts for which)
W25_LOOPS = W24A_LOOPS + [56] * 2 + [112]
WORDS = (1, 5, 3, 3, 5, 5, 1, 0)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
POINTS = [0, 1, -1, 2, -2, .5, -.5]
# B5^T as the kernel's transform states it (W25_XFORM), row j: the coefficients of prod_{k != j} (x - p_k)
B5T = np.array([[-1, 0, 5.25, 0, -5.25, 0, 1],
                [0, 1, 1, -4.25, -4.25, 1, 1], [0, -1, 1, 4.25, -4.25, -1, 1],
                [0, .5, .25, -2.5, -1.25, 2, 1], [0, -.5, .25, 2.5, -1.25, -2, 1],
                [0, 2, 4, -2.5, -5, .5, 1], [0, -2, 4, 2.5, -5, -.5, 1]], np.float64)
A5T = np.array([[p ** i for p in POINTS] for i in range(5)], np.float64)


def g5():
    out = np.zeros((7, 3))
    for j, p in enumerate(POINTS):
        nj = np.prod([p - q for k, q in enumerate(POINTS) if k != j])
        out[j] = [1 / nj, p / nj, p * p / nj]
    return out


def untile25(t, cout, cin):
    """the kernel's tiling [i][k-step][N-tile][ [lk][li][j = 0..3] | [lk][li][j = 4, 5] | [lk][li][j = 6] ] -> U [4, 7, Cout, Cin]"""
    t = t.reshape(4, cin // 4, cout // 16, 448)
    parts = [t[..., :256].reshape(4, cin // 4, cout // 16, 4, 16, 4), t[..., 256:384].reshape(4, cin // 4, cout // 16, 4, 16, 2),
             t[..., 384:].reshape(4, cin // 4, cout // 16, 4, 16, 1)]
    u = np.concatenate(parts, axis=-1)                                           # [i, ks, n, lk, li, j]
    return np.transpose(u, (0, 5, 2, 4, 1, 3)).reshape(4, 7, cout, cin)


def zero_layers(widths_in=RELEASED_IN, widths_out=RELEASED_OUT):
    return [(np.zeros((co, ci, 3, 3), np.float32), np.zeros(co, np.float32), l < 7) for l, (ci, co) in enumerate(zip(widths_in, widths_out))]


def test_the_ops_matrices_are_the_kernels():
    from buffer_amd import ops
    assert list(ops.F25_POINTS) == POINTS
    assert np.array_equal(ops.F25_B5T, B5T) and np.array_equal(ops.F25_A5T, A5T)
    assert np.allclose(ops.F25_G5, g5(), rtol=1e-15, atol=0)


def test_transform_identity_on_a_whole_map():
    """Y = A2^T [ sum_c U (.) (B2^T d B5) ] A5 over the 4 x 4 tiles of a padded 7 x 20 map equals the float64 correlation (row 7 dropped)"""
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal((3, 7, 20)), rng.standard_normal((5, 3, 3, 3))
    U = np.einsum('ia,ocab,jb->ijoc', G2, w, g5())
    xp = np.zeros((3, 10, 22))
    xp[:, 1:8, 1:21] = x
    xp[:, 1:8, 0], xp[:, 1:8, 21] = x[:, :, 19], x[:, :, 0]
    y = np.zeros((5, 8, 20))
    for ty in range(4):
        for tx in range(4):
            V = np.einsum('ia,cab,jb->ijc', B2T, xp[:, 2 * ty:2 * ty + 4, 5 * tx:5 * tx + 7], B5T)
            y[:, 2 * ty:2 * ty + 2, 5 * tx:5 * tx + 5] = np.einsum('ui,ijo,vj->ouv', A2T, np.einsum('ijoc,ijc->ijo', U, V), A5T)
    assert np.abs(y[:, :7] - correlate(x, w)).max() < 1e-12


@pytest.mark.parametrize('cout,cin', [(64, 48), (32, 64), (16, 4)])
def test_tile_weights_against_float64(cout, cin):
    """buf_winograd_f25_tile_weights: U = G2 g G5^T in fp64, rounded once, in the kernel's tiling; ops.winograd_f25_tile_weights bit for bit"""
    from buffer_amd import _lib, ops
    rng = np.random.default_rng(cout + cin)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    out = np.full(28 * cout * cin, np.nan, np.float32)
    assert _lib.lib().buf_winograd_f25_tile_weights(w.ctypes.data, cout, cin, out.ctypes.data) == 0
    want = np.einsum('ia,ocab,jb->ijoc', G2, w.astype(np.float64), g5())
    got = untile25(out, cout, cin)
    assert not np.isnan(out).any()
    # rounded once: within half an ulp of the float64 value (the nine products are summed in another order there: a few 1e-16 relative)
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)) * 0.5 + 1e-14)
    mine = ops.winograd_f25_tile_weights(w)
    assert mine.shape == out.shape and np.array_equal(mine.view(np.int32), out.view(np.int32))


def test_tile_weights_arguments():
    from buffer_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    x = C.addressof(buf)
    assert L.buf_winograd_f25_tile_weights(None, 16, 4, x) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_winograd_f25_tile_weights(x, 24, 4, x) == -1 and b'widths' in L.buf_last_error()
    assert L.buf_winograd_f25_tile_weights(x, 16, 6, x) == -1 and b'widths' in L.buf_last_error()


def test_argument_checks():
    """Both entry points validate before their first device call, so dummy pointers do."""
    from buffer_amd import _lib
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ptrs = (C.c_void_p * 8)(*[x] * 8)
    none = (C.c_void_p * 8)()
    own24 = (C.c_void_p * 8)(x, None, None, None, None, None, x, x)
    own25 = (C.c_void_p * 8)(x, x, None, None, x, x, x, x)                  # every 64- and 32-output layer of the released stack
    ok_in, ok_out, words = ints(*RELEASED_IN), ints(*RELEASED_OUT), ints(*WORDS)

    def both(ci, co, re_, w24, w25):
        out = []
        rc = L.buf_cylindrical_net_w25(x, 2, ptrs, ptrs, ci, co, re_, w24, w25, x, None)
        out.append((rc, L.buf_last_error()))
        rc = L.buf_cylindrical_net_split_safe_w25(x, 2, ptrs, ptrs, ptrs, ci, co, re_, w24, w25, None, x, None, None, x, None)
        out.append((rc, L.buf_last_error()))
        return out

    for w24, w25 in ((None, own25), (own24, None)):
        for rc, msg in both(ok_in, ok_out, words, w24, w25):
            assert rc == -1 and b"null argument" in msg
    # a set goes on layers with 64 or 32 outputs and Cin % 16 == 0 only
    for bad in (2, 3):
        w25 = (C.c_void_p * 8)(*[x if l == bad else None for l in range(8)])
        for rc, msg in both(ok_in, ok_out, words, none, w25):
            assert rc == -1 and b"takes no F(2x5) set" in msg, msg
    assert L.buf_cylindrical_net_w25_flags(ints(40, 64, 64, 128, 128, 64, 64, 32), ok_out, words, none, own25) == -1
    assert b"layer 0 (40 -> 64) takes no F(2x5) set" in L.buf_last_error()
    # the relu words and the F(2x4) sets keep the rules of buf_cylindrical_net_wg_all
    for rc, msg in both(ok_in, ok_out, ints(1, 5, 3, 3, 5, 8, 1, 0), own24, own25):
        assert rc == -1 and b"relu word" in msg
    for rc, msg in both(ok_in, ok_out, ints(1, 5, 1, 3, 5, 5, 1, 0), own24, own25):
        assert rc == -1 and b"every layer with 128 output channels" in msg
    for rc, msg in both(ok_in, ok_out, words, (C.c_void_p * 8)(None, x, None, None, None, None, None, None), own25):
        assert rc == -1 and b"takes no F(2x4) set of its own" in msg
    for rc, msg in both(ints(48, 72, 64, 128, 128, 64, 64, 32), ints(72, 64, 128, 128, 64, 64, 32, 32), words, none, none):
        assert rc == -1 and b"unsupported widths" in msg
    # a wider layer may follow a 32-output layer that runs on an F(2x5) or an F(2x4) set, and only such a one
    a_in, a_out = ints(48, 64, 32, 32, 64, 64, 64, 32), ints(64, 32, 32, 64, 64, 64, 32, 32)
    a_words = ints(1, 1, 1, 1, 5, 5, 1, 0)
    for rc, msg in both(a_in, a_out, a_words, none, (C.c_void_p * 8)(x, None, None, x, x, x, None, None)):
        assert rc == -1 and b"only 32-output layers may follow" in msg and b"layer 3 has unsupported widths 32 -> 64" in msg, msg
    flags = L.buf_cylindrical_net_w25_flags
    assert flags(a_in, a_out, a_words, none, (C.c_void_p * 8)(None, x, x, None, None, None, None, None)) == 0
    assert flags(a_in, a_out, a_words, (C.c_void_p * 8)(None, x, None, None, None, None, None, None), (C.c_void_p * 8)(None, None, x, None, None, None, None, None)) == 0
    # accepted: with and without F(2x4) sets beside, an F(2x5) set on a layer that carries the F(2x4) bit or a set, no set at all
    assert flags(ok_in, ok_out, words, own24, own25) == 0 and flags(ok_in, ok_out, words, none, own25) == 0
    assert flags(ok_in, ok_out, words, own24, none) == 0 and flags(ok_in, ok_out, words, none, none) == 0
    assert flags(ok_in, ok_out, words, none, None) == -1 and b"null argument" in L.buf_last_error()
    assert L.buf_cylindrical_net_w25(x, 0, ptrs, ptrs, ok_in, ok_out, words, none, none, x, None) == 0       # no patches: nothing is looked at
    assert L.buf_cylindrical_net_w25(x, -1, ptrs, ptrs, ok_in, ok_out, words, own24, own25, x, None) == -1 and b"npatch" in L.buf_last_error()
    assert L.buf_cylindrical_net_split_safe_w25(x, 2, ptrs, ptrs, ptrs, ok_in, ok_out, words, own24, own25, x, x, None, None, x, None) == -1
    assert b"head without desc" in L.buf_last_error()


def test_ops_defaults_and_explicit_arguments():
    """f25 picks the layers by output width; 'off' leaves every attribute of the net what it was; the F(2x4) buffers do not change."""
    from buffer_amd import ops
    layers = zero_layers()
    assert ops.F25_DEFAULT in ops.F25_PARTS
    want = {'all': [0, 1, 4, 5, 6, 7], 'out64': [0, 1, 4, 5], 'out32': [6, 7], 'off': []}
    net = ops.CylindricalNet(layers, 'cpu')
    assert net.f25_layers == want[ops.F25_DEFAULT] and list(net._re) == list(WORDS)
    for part, ls in want.items():
        net = ops.CylindricalNet(layers, 'cpu', f25=part)
        assert net.f25_layers == ls and list(net._re) == list(WORDS)
        assert [t is not None for t in net.wt25] == [l in ls for l in range(8)] and [bool(p) for p in net._w25p] == [l in ls for l in range(8)]
        assert all(t.numel() == 28 * layers[l][0].shape[0] * layers[l][0].shape[1] for l, t in enumerate(net.wt25) if t is not None)
        assert net.f24_layers == {'all': [0, 6, 7], 'out64': [0], 'out32': [6, 7], 'off': []}[ops.F24A_DEFAULT]
        assert [t.numel() for t in net.wt] == [(40 if f > 1 else 16) * w.shape[0] * w.shape[1] for (w, _, _), f in zip(layers, net._re)]
        split = ops.CylindricalNetSplit(layers, 'cpu', f25=part)
        assert not split.safe or split.f25_layers == ls
    assert ops.CylindricalNet(layers, 'cpu', f25=True).f25_layers == want['all'] and ops.CylindricalNet(layers, 'cpu', f25=False).f25_layers == []
    assert ops.CylindricalNet(layers, 'cpu', f24a='off', f25='out64').f24_layers == []
    # a Cin that is no multiple of 16 gets no set
    odd = zero_layers((40,) + RELEASED_IN[1:], RELEASED_OUT)
    assert ops.CylindricalNet(odd, 'cpu', f24a='off', f25='all').f25_layers == [1, 4, 5, 6, 7]
    # an explicit older form: no F(2x5) layers unless asked for, and then only with the default forms
    for kw in (dict(f24p=True), dict(f24k=True), dict(f24=True)):
        assert ops.CylindricalNet(layers, 'cpu', **kw).f25_layers == []
    assert ops.CylindricalNet(layers, 'cpu', f24p=True, f25='out64').f25_layers == want['out64']
    for kw in (dict(f24p=False), dict(f24k=False), dict(f24=False)):
        assert ops.CylindricalNet(layers, 'cpu', **kw).f25_layers == []
        with pytest.raises(ValueError):
            ops.CylindricalNet(layers, 'cpu', f25='all', **kw)
    for bad in ('some', 'out128'):
        with pytest.raises(ValueError):
            ops.CylindricalNet(layers, 'cpu', f25=bad)


def loop_stats(text):
    out = []
    for a, b in loops(text):
        ops = [op for _, op, _ in text[a:b + 1]]
        out.append(dict(mfma=sum(1 for o in ops if o.startswith('v_mfma')), valu=sum(1 for o in ops if o.startswith('v_') and not o.startswith('v_mfma')),
                        lds=sum(1 for o in ops if o.startswith('ds_read')), lds64=ops.count('ds_read_b64'), vmem=sum(1 for o in ops if o.startswith('buffer_load')),
                        acc=sum(1 for o in ops if o.startswith('v_accvgpr'))))
    return [s for s in out if s['mfma']]


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop (four k-steps per iteration), W25_LOOPS: every loop of W24A_LOOPS (tests/test_cyl_f24a_cpu.py) and, for
    the F(2x5) forms, ONE pass loop of 4 x 28 = 112 (64 outputs) and one of 4 x 14 = 56 built twice (32 outputs: LDS / global stores).
    The F(2x5) forms have no direct loop: no loop of 24 beyond those of the other forms.  The fused kernel holds every one of them, and
    no loop of 56 or 112 beyond these three (its loops outside the k-loops: tests/test_cyl_taps_cpu.py)."""
    asm, _ = code_object
    counts = mfma_per_loop(kernel_text(asm, name))
    print(f'MFMAs per k-loop of {name}:', counts)
    assert sorted(W25_LOOPS) == [24] * 6 + [32] * 12 + [48] * 7 + [56] * 2 + [96] + [112]
    assert beyond(W25_LOOPS, W24A_LOOPS) == ([56, 56, 112], [])
    assert beyond(counts, W25_LOOPS)[1] == [], counts
    assert [c for c in counts if c in (24, 56, 112)] == [24] * 6 + [56] * 2 + [112]


@pytest.mark.parametrize('name', KERNELS)
def test_the_new_pass_loops(code_object, name):
    """Per iteration four k-steps: two window rows of seven words each as four 4-byte-aligned LDS reads (32, none of them a ds_read_b64),
    four transforms of 28 vector instructions plus two address advances per k-step -- the issue's budget of 30 per k-step --, three
    buffer loads per N-tile and k-step, and no copies between the register files."""
    asm, _ = code_object
    new = [s for s in loop_stats(kernel_text(asm, name)) if s['mfma'] in (56, 112)]
    print(name, new)
    assert len(new) == 3
    for s in new:
        assert s['lds'] == 32 and s['lds64'] == 0 and s['acc'] == 0
        assert s['valu'] <= 4 * 30
        assert s['vmem'] == 4 * 3 * (s['mfma'] // 28)


def test_issued_count_of_the_released_stack():
    """28 per (k-step, N-tile) in the 64- and 32-output layers (352 units), 30 in the 128-output layers (384): 21 376 per patch, against
    the 22 080 of F(2x4) tiles in every layer."""
    units = {co: 0 for co in (32, 64, 128)}
    for ci, co in zip(RELEASED_IN, RELEASED_OUT):
        units[co] += (ci // 4) * (co // 16)
    assert units == {64: 304, 32: 48, 128: 384}
    assert 28 * (units[64] + units[32]) + 30 * units[128] == 21376 and 30 * sum(units.values()) == 22080
    assert 28 * units[64] + 30 * (units[32] + units[128]) == 21472 and 28 * units[32] + 30 * (units[64] + units[128]) == 21984
