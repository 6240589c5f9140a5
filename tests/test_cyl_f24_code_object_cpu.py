"""Code-object checks of the 128-output layers' Winograd F(2x4, 3x3) form (w24_layer_pair, csrc/convnet_w24.hip) in the fused kernel that
holds every layer form, k_cyl_net_w25t / k_cyl_net_w25t_rerun (cyl_net_w25t_body, csrc/convnet_w25t.hip), read off the gfx950 code object
of the in-tree library like tests/test_cyl_code_object_cpu.py; no GPU needed.

The layer forms were added one at a time, each with k-loops of its own in front of the same ladder.  Every form's test file keeps the list
of loops the body held when that form was its newest (W24_LOOPS here, then W24P_LOOPS, W24A_LOOPS, W25_LOOPS) and asserts that the fused
kernel still holds all of them and that its step added exactly the loops its docstring names; tests/test_cyl_taps_cpu.py asserts the
whole list (and the register and memory bounds of the kernel: its test_resources)."""
from collections import Counter

import pytest

from test_cyl_code_object_cpu import code_object, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)

KERNELS = ['k_cyl_net_w25t', 'k_cyl_net_w25t_rerun']

# MFMAs per k-loop (four k-steps per iteration) of the forms of k_cyl_net_wg: 64 outputs (wg_layer_msplit), four loops of 32 and a direct
# loop of 24; 32 outputs (wg_layer_mksplit, built twice: LDS / global stores), eight loops of 32 and two of 24
F22_LOOPS = [24] * 3 + [32] * 12
# ... and of the 128-output form: a pass issues the 6 column components of one M-tile for the N-tile pair, 12 per k-step: four loops of 48,
# and the direct round of the pair one loop of 48 -- 24 + 6 = 30 per (k-step, N-tile)
W24_LOOPS = F22_LOOPS + [48] * 5


def mfma_per_loop(text):
    """fp32 MFMAs of every k-loop of a kernel's text, ascending"""
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    return [c for c in counts if c]


def beyond(whole, part):
    """(what `whole` holds beyond `part`, what `part` holds and `whole` does not): two sorted lists, as multisets"""
    w, p = Counter(whole), Counter(part)
    return sorted((w - p).elements()), sorted((p - w).elements())


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop (four k-steps per iteration).  The 128-output form adds four pass loops of 48 and one direct loop of 48 to
    the loops of the 64- and 32-output forms of k_cyl_net_wg, and the fused kernel holds every one of them."""
    asm, _ = code_object
    counts = mfma_per_loop(kernel_text(asm, name))
    print(f'MFMAs per k-loop of {name}:', counts)
    assert W24_LOOPS == [24] * 3 + [32] * 12 + [48] * 5
    assert beyond(W24_LOOPS, F22_LOOPS) == ([48] * 5, [])
    assert beyond(counts, W24_LOOPS)[1] == [], counts
