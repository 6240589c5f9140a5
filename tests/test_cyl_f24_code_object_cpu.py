"""Code-object checks of k_cyl_net_w24 / k_cyl_net_w24_rerun (csrc/convnet_w24.hip: the descriptor CNN with its 128-output layers in the
Winograd F(2x4, 3x3) form), read off the gfx950 code object of the in-tree library like tests/test_cyl_code_object_cpu.py; no GPU needed."""
import re

import pytest

from test_cyl_code_object_cpu import code_object, kernel_meta, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)

KERNELS = ['k_cyl_net_w24', 'k_cyl_net_w24_rerun']


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
    assert not [op for _, op, _ in text if re.match(r'v_pk_(mul|add|fma)_f32', op)]
    assert not [op for _, op, _ in text if op.startswith('scratch_')]
    ls = loops(text)
    assert ls, 'no loop found: the disassembly format changed?'
    for a, b in ls:
        bad = [op for _, op, _ in text[a:b + 1] if op == 'ds_read2_b64']
        assert not bad, f'{len(bad)} ds_read2_b64 in the loop at {text[a][0]:#x}'


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop (four k-steps per iteration).  The 128-output form: a pass issues the 6 column components of one M-tile for
    the N-tile pair, 12 per k-step: four loops of 48, and the direct round of the pair one loop of 48 -- 24 + 6 = 30 per (k-step,
    N-tile).  The 64- and 32-output forms are those of k_cyl_net_wg: four loops of 32 and a direct loop of 24 each (the 32-output form is
    built twice: LDS / global stores)."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    counts = [c for c in counts if c]
    print(f'MFMAs per k-loop of {name}:', counts)
    assert counts == [24] * 3 + [32] * 12 + [48] * 5, counts
    assert sum(1 for _, op, _ in text if op.startswith('v_mfma')) == sum(counts)       # none outside the k-loops
