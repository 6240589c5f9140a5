"""Host side and code object of the pass-split form (w24p_layer_psplit, csrc/convnet_w24p.hip: the flagged 64-output layers of the
descriptor CNN split over the wavefronts by row component) in the fused kernel k_cyl_net_w25t / k_cyl_net_w25t_rerun: how the form is
chosen (an argument of buf_cylindrical_net_wg_form and buf_cylindrical_net_split_safe_form, not the relu word) and what the kernels compiled to, read off the gfx950 code object of the in-tree
library.  No GPU needed."""
import ctypes as C

import pytest

from test_cyl_code_object_cpu import code_object, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)
from test_cyl_f24_code_object_cpu import KERNELS, W24_LOOPS, beyond, mfma_per_loop
from test_cyl_f24k_cpu import RELEASED_IN, RELEASED_OUT, ints

# MFMAs per k-loop of the body whose newest form was the pass split (test_matrix_instruction_count says which form accounts for which)
W24P_LOOPS = [24] * 4 + [32] * 12 + [48] * 5 + [96]


def test_form_argument():
    """The launcher validates before its first device call, so dummy pointers do.  The form is an argument; the relu words keep their
    rules (words above 7 rejected whatever the form) and buf_cylindrical_net_wg_flags its three arguments."""
    from buffer_amd import _lib, ops
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ptrs = (C.c_void_p * 8)(*[x] * 8)
    ok_in, ok_out, words = ints(*RELEASED_IN), ints(*RELEASED_OUT), ints(1, 5, 3, 3, 5, 5, 1, 0)
    for form in (-2, 2, 8):
        assert L.buf_cylindrical_net_wg_form(x, 2, ptrs, ptrs, ok_in, ok_out, words, form, x, None) == -1 and b"form=" in L.buf_last_error()
        rc = L.buf_cylindrical_net_split_safe_form(x, 2, ptrs, ptrs, ptrs, ok_in, ok_out, words, form, None, x, None, None, x, None)
        assert rc == -1 and b"form=" in L.buf_last_error()
    for form in (-1, 0, 1):
        rc = L.buf_cylindrical_net_wg_form(x, 2, ptrs, ptrs, ok_in, ok_out, ints(1, 5, 3, 3, 5, 8, 1, 0), form, x, None)
        assert rc == -1 and b"F(2x4) flag" in L.buf_last_error()
        assert L.buf_cylindrical_net_wg_form(x, 0, ptrs, ptrs, ok_in, ok_out, words, form, x, None) == 0          # no patches: nothing to launch
    assert L.buf_cylindrical_net_wg_flags(ok_in, ok_out, words) == 0
    import numpy as np
    layers = [(np.zeros((co, ci, 3, 3), np.float32), np.zeros(co, np.float32), True) for ci, co in zip(RELEASED_IN, RELEASED_OUT)]
    for f24p in (True, False):
        net = ops.CylindricalNet(layers, 'cpu', f24p=f24p)
        assert net.form == int(f24p) and list(net._re) == [1, 5, 3, 3, 5, 5, 1, 1]
    assert ops.CylindricalNet(layers, 'cpu').form == int(ops.F24P_DEFAULT)


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop (four k-steps per iteration), one set of loops per layer form, W24P_LOOPS:
    * 128 outputs (w24_layer_pair): four pass loops of 48 and the pair's direct round, one loop of 48;
    * 64 outputs, flagged (w24p_layer_psplit): ONE pass loop of 96 (6 column components x 4 N-tiles x 4 k-steps: the wavefront's row
      component for the whole layer) and a direct loop of 24 (one N-tile);
    * 64 outputs, unflagged (wg_layer_msplit: layer 0): four loops of 32 and a direct loop of 24;
    * 32 outputs (wg_layer_mksplit), built twice (LDS / global stores): eight loops of 32 and two of 24.
    [24] x 4 + [32] x 12 + [48] x 5 + [96].  Per wavefront and k-step of a flagged layer 24 + 6, as in the K split: 22 848 per patch.
    Beyond W24_LOOPS (tests/test_cyl_f24_code_object_cpu.py) that is the pass-split form's own two loops, and the fused kernel holds every
    one of them (its loops outside the k-loops: tests/test_cyl_taps_cpu.py)."""
    asm, _ = code_object
    counts = mfma_per_loop(kernel_text(asm, name))
    print(f'MFMAs per k-loop of {name}:', counts)
    assert W24P_LOOPS == [24] * 4 + [32] * 12 + [48] * 5 + [96]
    assert beyond(W24P_LOOPS, W24_LOOPS) == ([24, 96], [])
    assert beyond(counts, W24P_LOOPS)[1] == [], counts


@pytest.mark.parametrize('name', KERNELS)
def test_the_pass_loop_carries_no_register_traffic(code_object, name):
    """The 96 accumulators of the pass loop live in accumulation registers and the filter ring and the operands in vector registers:
    nothing is copied between the two files inside the loop."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    big = [(a, b) for a, b in loops(text) if sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma')) == 96]
    assert len(big) == 1
    a, b = big[0]
    assert not [op for _, op, _ in text[a:b + 1] if op.startswith('v_accvgpr')]
    assert sum(1 for _, op, _ in text[a:b + 1] if op == 'ds_read_b64') == 24


def test_issued_count_of_the_released_stack():
    """Per flagged layer the four wavefronts together issue (24 + 6) x k-steps x 4 N-tiles... per wavefront 24 + 6 per k-step of the
    layer, the K split's figure: the stack stays at 22 848."""
    units = lambda ci, co: (ci // 4) * (co // 16)
    flagged = [(ci, co) for ci, co in zip(RELEASED_IN, RELEASED_OUT) if co == 64 and ci % 64 == 0]
    per_wavefront = [(24 + 6) * (ci // 4) for ci, co in flagged]
    assert [4 * p for p in per_wavefront] == [30 * units(ci, co) for ci, co in flagged]
    f24 = sum(units(ci, co) for ci, co in zip(RELEASED_IN, RELEASED_OUT) if co == 128 or (co == 64 and ci % 64 == 0))
    rest = sum(units(ci, co) for ci, co in zip(RELEASED_IN, RELEASED_OUT)) - f24
    assert (f24, rest) == (640, 96) and 30 * f24 + 38 * rest == 22848
