"""Host side and code object of k_cost_net_w24 / k_cost_net_w24_rerun (csrc/costnet_w24.hip: the cost net with F(2x4) tiles in layers 2
and 4 and the Winograd F(2x2) form in layer 6): what the kernels compiled to, read off the gfx950 code object of the in-tree library; the
three extra filter sets and the form argument of the ops classes; the argument checks of the new entry points; and the float32
restatement of the new arithmetic (tools/cost_f24_restate.py) at one match.  No GPU needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from test_cyl_code_object_cpu import ROOT, code_object, kernel_meta, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)

KERNELS = ['k_cost_net_w24', 'k_cost_net_w24_rerun']
SHAPES = [(32, 32, 3, 3, 3), (64, 32, 3, 3, 3), (64, 64, 3, 1, 3), (128, 64, 3, 1, 3), (128, 128, 3, 1, 3), (64, 128, 3, 1, 3),
          (64, 64, 3, 1, 3), (32, 64, 3, 1, 3), (32, 32, 3, 1, 3), (20, 32, 2, 1, 2)]


def random_layers(seed=0):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal(s) * np.sqrt(2.0 / np.prod(s[1:]))).astype(np.float32), (0.1 * rng.standard_normal(s[0])).astype(np.float32))
            for s in SHAPES]


@pytest.mark.parametrize('name', KERNELS)
def test_resources(code_object, name):
    """No scratch, no packed-fp32 instructions, both register kinds together within 256 (two workgroups per CU), and no LDS beside the
    dynamic buffer of CV_BUF floats, which two workgroups fit into a CU's 160 KB."""
    asm, notes = code_object
    m = kernel_meta(notes, name)
    print(name, m)
    assert m['private_segment_fixed_size'] == 0, 'scratch memory'
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    assert m['vgpr_count'] <= 256 and m['agpr_count'] <= 256          # .vgpr_count of the unified file counts both kinds
    assert m['group_segment_fixed_size'] == 0, 'static LDS beside the dynamic buffer'
    src = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'costnet.hip')).read()
    cv_buf = int(re.search(r'#define CV_BUF (\d+)', src).group(1))
    launch = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'cnn_launch.hip')).read()      # (the cost kernels' one launcher)
    assert launch.count('size_t lds = sizeof(float) * CV_BUF;') == 1 and 2 * 4 * cv_buf <= 160 * 1024
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
    """Static count per k-loop, four k-steps per iteration (the direct layers: one tap per iteration).  Every layer form the kernel can be
    switched to is in it once:
    * phase A.2 (layer 1, four chunks, a pair over one M-tile): 16 loops of 32;
    * layers 2 and 4 on F(2x4) tiles (cw24_layer -> w24_round): four pass loops each of 6 components x 2 N-tiles x 4 k-steps = 48;
    * layers 2 and 4 in the F(2x2) form (no set given; a pair over two M-tiles): four loops each of 64;
    * layer 3 (a pair over two M-tiles, then over the third): four loops of 64 and four of 32;
    * layer 5 (one N-tile, one M-tile), built twice (channel-major / position-major stores): eight loops of 16;
    * layer 6 in the Winograd form (cw_layer at one N-tile and one M-tile): four loops of 4 x 4 = 16;
    * layer 6 direct (three M-tiles, four channel groups per tap): one loop of 48; layers 7..9: 16, 8, 8.
    Outside the loops are only the two fully unrolled GEMMs of phase A.1, (30 + 18) groups x 4 k-steps x 2 N-tiles = 384, as in k_cost_net
    (cv_gemm_static has no loop to be inside of)."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    counts = [c for c in counts if c]
    print(f'MFMAs per k-loop of {name}:', counts)
    assert counts == [8] * 2 + [16] * 13 + [32] * 20 + [48] * 9 + [64] * 12, counts
    total = sum(1 for _, op, _ in text if op.startswith('v_mfma'))
    assert total - sum(counts) == (30 + 18) * 4 * 2
    parent = kernel_text(asm, 'k_cost_net')
    in_loops = sum(sum(1 for _, op, _ in parent[a:b + 1] if op.startswith('v_mfma')) for a, b in loops(parent))
    assert sum(1 for _, op, _ in parent if op.startswith('v_mfma')) - in_loops == (30 + 18) * 4 * 2


@pytest.mark.parametrize('name', KERNELS)
def test_the_f24_pass_loops(code_object, name):
    """The eight pass loops of layers 2 and 4: per iteration four k-steps of two window rows of six words (24 ds_read_b64) and 48 MFMAs, no
    copies between the register files."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    hit = []
    for a, b in loops(text):
        ops = [op for _, op, _ in text[a:b + 1]]
        if sum(1 for o in ops if o.startswith('v_mfma')) == 48 and ops.count('ds_read_b64') == 24:
            hit.append(sum(1 for o in ops if o.startswith('v_accvgpr')))
    assert hit == [0] * 8, hit


def test_issued_count_per_match():
    """30 384 -> 26 608 issued matrix instructions per match (four wavefronts): the table of profiles/cost_f24_ab.md."""
    k_steps = {2: 16, 4: 32, 6: 16}
    f22 = {l: 4 * 16 * 2 * 2 * k_steps[l] for l in (2, 4)}                    # wavefronts x components x N-tiles x M-tiles x k-steps
    assert f22 == {2: 4096, 4: 8192}
    new = {2: 4 * 24 * 2 * k_steps[2], 4: 4 * 24 * 2 * k_steps[4], 6: 4 * 16 * k_steps[6]}      # one M-tile per wavefront
    assert new == {2: 3072, 4: 6144, 6: 1024}
    direct6 = 4 * 3 * 9 * 4 * 4                                               # wavefronts x M-tiles x taps x channel groups x k-steps
    assert direct6 == 1728
    assert 30384 - (f22[2] - new[2]) - (f22[4] - new[4]) - (direct6 - new[6]) == 26608


def test_filter_sets_and_form_argument():
    """The three sets are buf_winograd_f24_tile_weights / winograd_tile_weights (group 1) of the sliced filters, live in buffers of their
    own, and a part that is not selected passes a null pointer: that layer runs as in k_cost_net.  The ten existing buffers do not change."""
    from buffer_amd import _lib, ops
    L = _lib.lib()
    layers = random_layers(3)
    assert ops.COST_F24_DEFAULT in ops.COST_F24_PARTS
    want = {'all': (2, 4, 6), 'l2': (2,), 'l4': (4,), 'l6': (6,), 'off': ()}
    off = ops.CostVolumeNet(layers, 'cpu', f24='off')
    assert off.parts == () and [bool(p) for p in off._fp] == [False] * 3
    for part, ls in want.items():
        net = ops.CostVolumeNet(layers, 'cpu', f24=part)
        assert net.parts == ls
        assert [t is not None for t in net.wt24] == [l in ls for l in (2, 4, 6)] == [bool(p) for p in net._fp]
        for a, b in zip(net.wt, off.wt):
            assert np.array_equal(a.numpy(), b.numpy())
        for l, t in zip((2, 4, 6), net.wt24):
            if t is None:
                continue
            w2d = np.ascontiguousarray(layers[l][0][:, :, :, 0, :])
            cout, cin = w2d.shape[:2]
            if l == 6:
                ref = np.empty(16 * cout * cin, np.float32)
                assert L.buf_winograd_tile_filters(w2d.ctypes.data, cout, cin, 1, 4, ref.ctypes.data) == 0
                assert np.array_equal(ref, ops.winograd_tile_weights(w2d, ng=1))
            else:
                ref = np.empty(24 * cout * cin, np.float32)
                assert L.buf_winograd_f24_tile_weights(w2d.ctypes.data, cout, cin, ref.ctypes.data) == 0
            assert t.numel() == ref.size and np.array_equal(t.numpy(), ref)
    assert ops.CostVolumeNet(layers, 'cpu').parts == want[ops.COST_F24_DEFAULT]
    assert ops.CostVolumeNet(layers, 'cpu', f24=True).parts == (2, 4, 6) and ops.CostVolumeNet(layers, 'cpu', f24=False).parts == ()
    split = ops.CostVolumeNetSplit(layers, 'cpu', f24='l4')
    assert split.parts == (4,) and (not split.safe or split.f32.parts == (4,))
    with pytest.raises(ValueError):
        ops.CostVolumeNet(layers, 'cpu', f24='l3')


def test_argument_checks():
    """The new entry points validate before their first device call, so dummy pointers do; no matches: nothing is looked at."""
    from buffer_amd import _lib
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ten = (C.c_void_p * 10)(*[x] * 10)
    eleven = (C.c_void_p * 11)(*[x] * 11)
    sets = (C.c_void_p * 3)()
    assert L.buf_cost_volume_net_w24(x, x, 0, ten, ten, sets, x, None) == 0
    assert L.buf_cost_volume_net_w24(x, x, -1, ten, ten, sets, x, None) == -1 and b'm=-1' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24(x, x, 2, ten, ten, None, x, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24(x, x, 2, (C.c_void_p * 10)(), ten, sets, x, None) == -1 and b'null weights for layer 0' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24_gather(x, 7, x, x, 0, ten, ten, sets, x, None) == 0
    assert L.buf_cost_volume_net_w24_gather(x, 6, x, x, 2, ten, ten, sets, x, None) == -1 and b'ele_n=6' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24_gather(x, 7, x, x, 2, ten, ten, None, x, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_split_safe_w24(x, x, 7, None, None, 0, eleven, ten, ten, ten, sets, x, None, x, None) == 0
    assert L.buf_cost_volume_net_split_safe_w24(x, x, 7, None, None, 2, eleven, ten, ten, ten, None, x, None, x, None) == -1
    assert b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_split_safe_w24(x, x, 7, x, None, 2, eleven, ten, ten, ten, sets, x, None, x, None) == -1
    assert b'one row list without the other' in L.buf_last_error()


def test_restatement_meets_its_bound_at_one_match():
    """tools/cost_f24_restate.py, the float32 restatement the kernel was written from: at the first match of tests/golden/match_tiny.npz the
    new forms stay below 1e-4 of the network in float64 (ind in [0, 20)) -- the bound of the kernel's GPU tests -- and the float64 path of
    the restatement is the recorded ind of the fixture.  (Over all 40 matches and 70 random maps: profiles/cost_f24_ab.md.)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import cost_f24_restate as r
    finally:
        sys.path.pop(0)
    layers = r.released_layers()
    se, te = r.golden_matches()
    ref = r.ind_of(se[0], te[0], layers, 'f64')
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'match_tiny.npz'))['ind'][0]
    assert abs(ref - gold) <= 1e-4 * max(1.0, abs(gold)) + 2e-4
    for form in ('new', (2,), (4,), (6,), 'parent'):
        e = abs(r.ind_of(se[0], te[0], layers, form) - ref)
        print(f'restatement, forms {form}: |ind - ind64| = {e:.2e}')
        assert e < 1e-4
