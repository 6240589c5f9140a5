"""Host side and code object of k_cyl_net_w24p / k_cyl_net_w24p_rerun (csrc/convnet_w24p.hip: the flagged 64-output layers of the
descriptor CNN split over the wavefronts by row component): how the form is chosen (an argument of buf_cylindrical_net_wg_form and
buf_cylindrical_net_split_safe_form, not the relu word) and what the kernels compiled to, read off the gfx950 code object of the in-tree
library.  No GPU needed."""
import ctypes as C
import re

import pytest

from test_cyl_code_object_cpu import code_object, kernel_meta, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)
from test_cyl_f24k_cpu import RELEASED_IN, RELEASED_OUT, ints

KERNELS = ['k_cyl_net_w24p', 'k_cyl_net_w24p_rerun']


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
def test_resources(code_object, name):
    asm, notes = code_object
    m = kernel_meta(notes, name)
    print(name, m)
    assert m['private_segment_fixed_size'] == 0, 'scratch memory'
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    assert m['vgpr_count'] <= 256 and m['agpr_count'] <= 256          # the unified file: two workgroups per CU
    assert m['group_segment_fixed_size'] == 0, 'static LDS beside the dynamic 80 KB buffer'
    text = kernel_text(asm, name)
    assert not [op for _, op, _ in text if re.match(r'v_pk_\w+_f32', op)]
    assert not [op for _, op, _ in text if op.startswith('scratch_')]
    ls = loops(text)
    assert ls, 'no loop found: the disassembly format changed?'
    for a, b in ls:
        bad = [op for _, op, _ in text[a:b + 1] if op == 'ds_read2_b64']
        assert not bad, f'{len(bad)} ds_read2_b64 in the loop at {text[a][0]:#x}'


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop (four k-steps per iteration), one set of loops per layer form in the kernel:
    * 128 outputs (w24_layer_pair): four pass loops of 48 and the pair's direct round, one loop of 48;
    * 64 outputs, flagged (w24p_layer_psplit): ONE pass loop of 96 (6 column components x 4 N-tiles x 4 k-steps: the wavefront's row
      component for the whole layer) and a direct loop of 24 (one N-tile);
    * 64 outputs, unflagged (wg_layer_msplit: layer 0): four loops of 32 and a direct loop of 24;
    * 32 outputs (wg_layer_mksplit), built twice (LDS / global stores): eight loops of 32 and two of 24.
    [24] x 4 + [32] x 12 + [48] x 5 + [96].  Per wavefront and k-step of a flagged layer 24 + 6, as in the K split: 22 848 per patch."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    counts = [c for c in counts if c]
    print(f'MFMAs per k-loop of {name}:', counts)
    assert counts == [24] * 4 + [32] * 12 + [48] * 5 + [96], counts
    assert sum(1 for _, op, _ in text if op.startswith('v_mfma')) == sum(counts)       # none outside the k-loops


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
