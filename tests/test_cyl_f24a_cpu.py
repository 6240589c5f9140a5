"""Host side and code object of the layer forms on F(2x4) sets of their own in the fused kernel k_cyl_net_w25t / k_cyl_net_w25t_rerun
(csrc/convnet_w24a.hip: F(2x4) tiles in every layer of the descriptor CNN -- layer 0 through the pass-split form of the 64-output layers, the 32-output layers through a pass split over one N-tile
pair): the argument checks of the new entry points, what the two ops classes run with and without a form argument, and what the
kernels compiled to, read off the gfx950 code object of the in-tree library.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from test_cyl_code_object_cpu import code_object, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)
from test_cyl_f24_code_object_cpu import KERNELS, beyond, mfma_per_loop
from test_cyl_f24k_cpu import RELEASED_IN, RELEASED_OUT, ints
from test_cyl_f24p_cpu import W24P_LOOPS

# MFMAs per k-loop of the body whose newest forms were these (test_matrix_instruction_count says which form accounts for which)
W24A_LOOPS = [24] * 6 + [32] * 12 + [48] * 7 + [96]
WORDS = (1, 5, 3, 3, 5, 5, 1, 0)


def zero_layers(widths_in=RELEASED_IN, widths_out=RELEASED_OUT):
    return [(np.zeros((co, ci, 3, 3), np.float32), np.zeros(co, np.float32), l < 7) for l, (ci, co) in enumerate(zip(widths_in, widths_out))]


def test_argument_checks():
    """Both entry points validate before their first device call, so dummy pointers do."""
    from buffer_amd import _lib
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ptrs = (C.c_void_p * 8)(*[x] * 8)
    none = (C.c_void_p * 8)()
    own = (C.c_void_p * 8)(x, None, None, None, None, None, x, x)          # layer 0 and the two 32-output layers
    ok_in, ok_out, words = ints(*RELEASED_IN), ints(*RELEASED_OUT), ints(*WORDS)

    def both(ci, co, re_, w24):
        """(return codes, messages) of the two entry points on the same stack"""
        out = []
        rc = L.buf_cylindrical_net_wg_all(x, 2, ptrs, ptrs, ci, co, re_, w24, x, None)
        out.append((rc, L.buf_last_error()))
        rc = L.buf_cylindrical_net_split_safe_all(x, 2, ptrs, ptrs, ptrs, ci, co, re_, w24, None, x, None, None, x, None)
        out.append((rc, L.buf_last_error()))
        return out

    for rc, msg in both(ok_in, ok_out, words, None):
        assert rc == -1 and b"null argument" in msg
    # the relu words keep the rules of buf_cylindrical_net_wg: words above 7, a flag on the wrong layer
    for rc, msg in both(ok_in, ok_out, ints(1, 5, 3, 3, 5, 8, 1, 0), own):
        assert rc == -1 and b"relu word" in msg
    for rc, msg in both(ok_in, ok_out, ints(1, 5, 1, 3, 5, 5, 1, 0), own):
        assert rc == -1 and b"every layer with 128 output channels" in msg
    # a set of its own goes on an unflagged layer with 64 or 32 outputs only
    for bad in (1, 2):
        w24 = (C.c_void_p * 8)(*[x if l == bad else None for l in range(8)])
        for rc, msg in both(ok_in, ok_out, words, w24):
            assert rc == -1 and b"takes no F(2x4) set of its own" in msg, msg
    # widths: the rules of buf_cylindrical_net_wg ...
    for rc, msg in both(ints(48, 72, 64, 128, 128, 64, 64, 32), ints(72, 64, 128, 128, 64, 64, 32, 32), words, own):
        assert rc == -1 and b"unsupported widths" in msg
    # ... but a wider layer may follow a 32-output layer that runs the new form, and only such a one
    a_in, a_out = ints(48, 64, 32, 32, 64, 64, 64, 32), ints(64, 32, 32, 64, 64, 64, 32, 32)
    a_words = ints(1, 1, 1, 1, 5, 5, 1, 0)
    assert L.buf_cylindrical_net_wg_supports(a_in, a_out) == -1
    for rc, msg in both(a_in, a_out, a_words, none):
        assert rc == -1 and b"only 32-output layers may follow" in msg
    a_own = (C.c_void_p * 8)(x, x, x, None, None, None, x, x)
    assert L.buf_cylindrical_net_wg_all(x, 0, ptrs, ptrs, a_in, a_out, a_words, none, x, None) == 0             # no patches: nothing is looked at
    # the rule holds to the end of the stack, not for the direct successor only: the older 32-output form leaves partial sums in zero words
    # that a LATER layer with more than 64 input channels reads as padding.  Layer 0 without a set, layer 1 with one, wider layers behind
    c_in, c_out = ints(64, 32, 32, 64, 128, 64, 32, 32), ints(32, 32, 64, 128, 64, 32, 32, 32)
    c_words = ints(1, 1, 1, 3, 5, 1, 1, 0)
    for w24 in ((C.c_void_p * 8)(None, x, None, None, None, None, None, None), (C.c_void_p * 8)(None, x, x, None, None, x, x, x)):
        for rc, msg in both(c_in, c_out, c_words, w24):
            assert rc == -1 and b"only 32-output layers may follow" in msg and b"layer 2 has unsupported widths 32 -> 64" in msg, msg
    # what is accepted (host only): stack A with a set for every 32-output layer; a 32-output layer without one at the END of a stack
    assert L.buf_cylindrical_net_wg_all_flags(a_in, a_out, a_words, a_own) == 0
    assert L.buf_cylindrical_net_wg_all_flags(ok_in, ok_out, words, own) == 0 and L.buf_cylindrical_net_wg_all_flags(ok_in, ok_out, words, none) == 0
    assert L.buf_cylindrical_net_wg_all_flags(ok_in, ok_out, words, (C.c_void_p * 8)(x, None, None, None, None, None, x, None)) == 0
    assert L.buf_cylindrical_net_wg_all_flags(ok_in, ok_out, words, (C.c_void_p * 8)(x, None, None, None, None, None, None, x)) == 0
    assert L.buf_cylindrical_net_wg_all_flags(c_in, c_out, c_words, (C.c_void_p * 8)(x, x, None, None, None, x, x, x)) == 0
    assert L.buf_cylindrical_net_wg_all_flags(c_in, c_out, c_words, (C.c_void_p * 8)(None, x, None, None, None, None, None, None)) == -1
    assert L.buf_cylindrical_net_wg_all_flags(ok_in, ok_out, words, None) == -1 and b"null argument" in L.buf_last_error()
    assert L.buf_cylindrical_net_wg_all(x, -1, ptrs, ptrs, ok_in, ok_out, words, own, x, None) == -1 and b"npatch" in L.buf_last_error()
    assert L.buf_cylindrical_net_split_safe_all(x, 2, ptrs, ptrs, ptrs, ok_in, ok_out, words, own, x, x, None, None, x, None) == -1
    assert b"head without desc" in L.buf_last_error()
    # the existing entry points keep their rules
    assert L.buf_cylindrical_net_wg_form(x, 2, ptrs, ptrs, ok_in, ok_out, words, 2, x, None) == -1 and b"form=" in L.buf_last_error()
    assert L.buf_cylindrical_net_wg_form(x, 2, ptrs, ptrs, ok_in, ok_out, ints(1, 5, 3, 3, 5, 8, 1, 0), 1, x, None) == -1
    assert L.buf_cylindrical_net_wg_flags(a_in, a_out, a_words) == -1 and L.buf_cylindrical_net_wg_flags(ok_in, ok_out, words) == 0


def test_ops_defaults_and_explicit_arguments():
    """No form argument -> a set of its own for layer 0 and the 32-output layers; an explicit f24, f24k or f24p -> exactly the
    arguments of the stacks without such sets.  The relu words and the per-layer buffers are the same either way."""
    from buffer_amd import ops
    layers = zero_layers()
    assert ops.F24A_DEFAULT in ops.F24A_PARTS
    want = {'all': [0, 6, 7], 'out64': [0], 'out32': [6, 7], 'off': [], None: []}
    net = ops.CylindricalNet(layers, 'cpu')
    assert net.form == int(ops.F24P_DEFAULT) and list(net._re) == list(WORDS)
    assert net.f24_layers == want[ops.F24A_DEFAULT] and net.f24_all == (ops.F24A_DEFAULT == 'all')
    for part, ls in want.items():
        if part is None:
            continue
        net = ops.CylindricalNet(layers, 'cpu', f24a=part)
        assert net.f24_layers == ls and net.f24_all == (part == 'all') and list(net._re) == list(WORDS)
        assert [t is not None for t in net.wt24] == [l in ls for l in range(8)]
        assert all(t.numel() == 24 * layers[l][0].shape[0] * layers[l][0].shape[1] for l, t in enumerate(net.wt24) if t is not None)
        assert [bool(p) for p in net._w24p] == [l in ls for l in range(8)]
        # the existing buffers do not change: the F(2x2) set, and behind it the F(2x4) set of the flagged layers only
        assert [t.numel() for t in net.wt] == [(40 if f > 1 else 16) * w.shape[0] * w.shape[1] for (w, _, _), f in zip(layers, net._re)]
    split = ops.CylindricalNetSplit(layers, 'cpu')
    assert split.form == int(ops.F24P_DEFAULT)
    if split.safe:
        assert split.f24_layers == want[ops.F24A_DEFAULT] and list(split._re_safe) == list(WORDS)
    for kw, form, re_ in ((dict(f24p=True), 1, list(WORDS)), (dict(f24p=False), 0, list(WORDS)),
                          (dict(f24k=False), int(ops.F24P_DEFAULT), [1, 1, 3, 3, 1, 1, 1, 0]), (dict(f24k=True), int(ops.F24P_DEFAULT), list(WORDS))):
        net = ops.CylindricalNet(layers, 'cpu', **kw)
        assert net.form == form and list(net._re) == re_ and net.f24_layers == [] and not net.f24_all
        split = ops.CylindricalNetSplit(layers, 'cpu', **kw)
        assert split.form == form and split.f24_layers == [] and (not split.safe or list(split._re_safe) == re_)
    net = ops.CylindricalNet(layers, 'cpu', f24=False)
    assert list(net._re) == [1] * 7 + [0] and net.f24_layers == []
    with pytest.raises(ValueError):
        ops.CylindricalNet(layers, 'cpu', f24a='some')
    with pytest.raises(ValueError):
        ops.CylindricalNet(layers, 'cpu', f24p=False, f24a='all')


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop (four k-steps per iteration), one set of loops per layer form, W24A_LOOPS:
    * 128 outputs (w24_layer_pair): four pass loops of 48 and the pair's direct round, one loop of 48;
    * 64 outputs on an F(2x4) set (w24p_layer_psplit): ONE pass loop of 96 and a direct loop of 24 (one N-tile);
    * 32 outputs on an F(2x4) set (w24a_layer_psplit32), built twice (LDS / global stores): ONE pass loop of 48 (6 column components x
      2 N-tiles x 4 k-steps) and a direct loop of 24 (one N-tile, run over half of K);
    * the F(2x2) forms for layers without such a set: 64 outputs (wg_layer_msplit), four loops of 32 and a direct loop of 24; 32 outputs
      (wg_layer_mksplit, built twice), eight loops of 32 and two of 24.
    [24] x (1 + 2 + 1 + 2) + [32] x (4 + 8) + [48] x (5 + 2) + [96].  Beyond W24P_LOOPS (tests/test_cyl_f24p_cpu.py) that is the 32-output
    form's pass loop and direct loop, twice, and the fused kernel holds every one of them (its loops outside the k-loops:
    tests/test_cyl_taps_cpu.py)."""
    asm, _ = code_object
    counts = mfma_per_loop(kernel_text(asm, name))
    print(f'MFMAs per k-loop of {name}:', counts)
    assert W24A_LOOPS == [24] * 6 + [32] * 12 + [48] * 7 + [96]
    assert beyond(W24A_LOOPS, W24P_LOOPS) == ([24] * 2 + [48] * 2, [])
    assert beyond(counts, W24A_LOOPS)[1] == [], counts


@pytest.mark.parametrize('name', KERNELS)
def test_the_new_pass_loop(code_object, name):
    """The pass loops of the 32-output form: per iteration four k-steps of two window rows (24 ds_read_b64), four transforms of 18 vector
    instructions (plus the two address advances), 48 MFMAs, and no copies between the register files.  They are the two loops of 48 MFMAs
    whose vector-instruction count is the 96-loop's (the same transform): the loops of the 128-output layers carry window selects."""
    asm, _ = code_object
    text = kernel_text(asm, name)

    def stats(a, b):
        ops = [op for _, op, _ in text[a:b + 1]]
        return dict(mfma=sum(1 for o in ops if o.startswith('v_mfma')), valu=sum(1 for o in ops if o.startswith('v_') and not o.startswith('v_mfma')),
                    lds=ops.count('ds_read_b64'), acc=sum(1 for o in ops if o.startswith('v_accvgpr')))
    all_loops = [stats(a, b) for a, b in loops(text)]
    big = [s for s in all_loops if s['mfma'] == 96]
    assert len(big) == 1 and big[0]['lds'] == 24 and big[0]['acc'] == 0
    new = [s for s in all_loops if s['mfma'] == 48 and s['lds'] == 24 and s['acc'] == 0 and s['valu'] == big[0]['valu']]
    print(name, big, new)
    assert len(new) == 2 and new[0]['valu'] == 4 * 18 + 2


def test_issued_count_of_the_released_stack():
    """Per (k-step, N-tile) 24 + 6 in every layer: in the 32-output form each wavefront issues 12 per k-step in the pass and 6 on half of
    the k-steps in the direct round, (12 + 3) x 4 = 60 for the two N-tiles.  30 x 736 = 22 080 for the released widths."""
    units = [(ci // 4) * (co // 16) for ci, co in zip(RELEASED_IN, RELEASED_OUT)]
    assert sum(units) == 736 and 30 * sum(units) == 22080
    for ci, co in zip(RELEASED_IN, RELEASED_OUT):
        k4 = ci // 4
        if co == 32:
            assert ci % 32 == 0 and 4 * (12 * k4 + 6 * (k4 // 2)) == 30 * k4 * 2
        elif co == 64:
            assert ci % 16 == 0 and 4 * (24 * k4 + 6 * k4) == 30 * k4 * 4
        else:
            assert 4 * (4 * 12 * k4 + 12 * k4) == 30 * k4 * 8
