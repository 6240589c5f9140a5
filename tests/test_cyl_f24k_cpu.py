"""Host side and code object of k_cyl_net_w24k / k_cyl_net_w24k_rerun (csrc/convnet_w24k.hip: the descriptor CNN with F(2x4, 3x3) tiles
in its 64-output layers of Cin % 64 == 0 as well, K split over the wavefront pairs): the rules of the flag (bit 2 of the relu word,
BUF_CYL_F24K) and what the kernels compiled to, read off the gfx950 code object of the in-tree library.  No GPU needed."""
import ctypes as C
import re

import pytest

from test_cyl_code_object_cpu import code_object, kernel_meta, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)

KERNELS = ['k_cyl_net_w24k', 'k_cyl_net_w24k_rerun']
RELEASED_IN, RELEASED_OUT = (48, 64, 64, 128, 128, 64, 64, 32), (64, 64, 128, 128, 64, 64, 32, 32)


def ints(*v):
    return (C.c_int * 8)(*v)


def test_flag_rules():
    """The launcher validates before its first device call, so dummy pointers do (as in test_winograd_f24_cpu); what it ACCEPTS is asked
    of buf_cylindrical_net_wg_flags, the same statement of the rules without the launch behind it."""
    from buffer_amd import _lib, ops
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ptrs = (C.c_void_p * 8)(*[x] * 8)
    ok_in, ok_out = ints(*RELEASED_IN), ints(*RELEASED_OUT)
    assert ops.F24K_FLAG == 4 and ops.F24_FLAG == 2
    for words in ((1, 5, 3, 3, 5, 5, 1, 0), (1, 1, 3, 3, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, 1, 0), (1, 5, 3, 3, 1, 5, 1, 0), (0, 4, 2, 2, 4, 4, 0, 0)):
        assert L.buf_cylindrical_net_wg_flags(ok_in, ok_out, ints(*words)) == 0, (words, L.buf_last_error())
    rejected = {
        'bit 2 on layer 0 (48 -> 64)': (5, 5, 3, 3, 5, 5, 1, 0),
        'bit 2 on a 32-output layer': (1, 5, 3, 3, 5, 5, 5, 0),
        'bit 2 on the last 32-output layer': (1, 5, 3, 3, 5, 5, 1, 4),
        'bit 2 on a 128-output layer': (1, 5, 7, 3, 5, 5, 1, 0),
        'bit 2 instead of bit 1 on a 128-output layer': (1, 5, 5, 3, 5, 5, 1, 0),
        'bit 2 while a 128-output layer lacks bit 1': (1, 5, 3, 1, 5, 5, 1, 0),
        'bit 2 while no 128-output layer has bit 1': (1, 5, 1, 1, 1, 1, 1, 0),
        'bits 1 and 2 on a 64-output layer': (1, 7, 3, 3, 5, 5, 1, 0),
        'a word of 8': (1, 5, 3, 3, 5, 8, 1, 0),
        'a word of 8 in an otherwise unflagged stack': (1, 1, 1, 1, 1, 1, 1, 8),
    }
    for why, words in rejected.items():
        assert L.buf_cylindrical_net_wg_flags(ok_in, ok_out, ints(*words)) == -1 and b"F(2x4) flag" in L.buf_last_error(), why
        rc = L.buf_cylindrical_net_wg(x, 2, ptrs, ptrs, ok_in, ok_out, ints(*words), x, None)
        assert rc == -1 and b"F(2x4) flag" in L.buf_last_error(), why
    # buf_cylindrical_net_split_safe checks the same rules before its memset and the split kernel
    rc = L.buf_cylindrical_net_split_safe(x, 2, ptrs, ptrs, ptrs, ok_in, ok_out, ints(1, 5, 3, 3, 5, 8, 1, 0), None, x, None, None, x, None)
    assert rc == -1 and b"F(2x4) flag" in L.buf_last_error()
    # the width rules come first
    rc = L.buf_cylindrical_net_wg(x, 2, ptrs, ptrs, ints(40, 64, 64, 128, 128, 64, 64, 32), ok_out, ints(1, 5, 3, 3, 5, 5, 1, 0), x, None)
    assert rc == -1 and b"unsupported widths" in L.buf_last_error()
    assert L.buf_cylindrical_net_wg_flags(ints(40, 64, 64, 128, 128, 64, 64, 32), ok_out, ints(1, 5, 3, 3, 5, 5, 1, 0)) == -1
    # Cin = 32 is no multiple of 64: 32 -> 64 may not carry the bit, 128 -> 64 and 64 -> 64 of the second stack of the GPU tests may
    si, so = ints(32, 64, 128, 128, 64, 64, 32, 32), ints(64, 128, 128, 64, 64, 32, 32, 32)
    assert L.buf_cylindrical_net_wg_flags(si, so, ints(1, 3, 3, 5, 5, 1, 1, 0)) == 0
    assert L.buf_cylindrical_net_wg_flags(si, so, ints(5, 3, 3, 5, 5, 1, 1, 0)) == -1 and b"F(2x4) flag" in L.buf_last_error()


def test_ops_flags_the_eligible_layers():
    import numpy as np
    from buffer_amd import ops
    for (cout, cin), flag in {(64, 64): 4, (64, 128): 4, (64, 48): 0, (64, 32): 0, (128, 64): 2, (128, 128): 2, (32, 64): 0}.items():
        w = np.zeros((cout, cin, 3, 3), np.float32)
        wt, f = ops.cyl_layer_filters(w)
        assert f == flag and wt.size == (40 if flag else 16) * cout * cin, (cout, cin)
        wt, f = ops.cyl_layer_filters(w, f24k=False)
        assert f == (flag & 2) and wt.size == (40 if f else 16) * cout * cin, (cout, cin)


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
    * 128 outputs (w24_layer_pair): a pass issues the 6 column components of the one M-tile for the N-tile pair, 12 per k-step: four
      loops of 48, and the direct round of the pair one loop of 48;
    * 64 outputs, flagged (w24k_layer_ksplit): the same two rounds over half of K: again four loops of 48 and one of 48;
    * 64 outputs, unflagged (wg_layer_msplit: layer 0): four loops of 32 (4 components x 2 N-tiles x 4 k-steps) and a direct loop of 24
      (one N-tile);
    * 32 outputs (wg_layer_mksplit), built twice (LDS / global stores): eight loops of 32 and two of 24.
    [24] x 3 + [32] x 12 + [48] x 10.  Per (k-step, N-tile) that is 24 + 6 = 30 in the flagged forms and 38 in the others: 22 848 per
    patch of the released stack."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    counts = [c for c in counts if c]
    print(f'MFMAs per k-loop of {name}:', counts)
    assert counts == [24] * 3 + [32] * 12 + [48] * 10, counts
    assert sum(1 for _, op, _ in text if op.startswith('v_mfma')) == sum(counts)       # none outside the k-loops


def test_issued_count_of_the_released_stack():
    units = lambda ci, co: (ci // 4) * (co // 16)
    f24 = sum(units(ci, co) for ci, co in zip(RELEASED_IN, RELEASED_OUT) if co == 128 or (co == 64 and ci % 64 == 0))
    rest = sum(units(ci, co) for ci, co in zip(RELEASED_IN, RELEASED_OUT)) - f24
    assert (f24, rest) == (640, 96) and 30 * f24 + 38 * rest == 22848
