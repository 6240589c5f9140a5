"""Host side and code object of k_cost_net_w24b / k_cost_net_w24b_rerun, the cost net's one kernel pair (csrc/costnet_body.hip: every
layer form in one body), and the forms of csrc/costnet_w24b.hip in it -- layer 1 on F(2x4) tiles, one k' plane resident at a time, and
layer 3 as F(2x4) rows with an F(2x2) tail: what the kernels compiled to, read off the gfx950 code object of the in-tree library; that
they are the only fp32 cost-net kernels and have one launch path; the two extra filter sets and the form argument f24b= of the ops
classes; the argument checks of the *_w24b entry points; and the float32 restatement of the arithmetic (tools/cost_f24b_restate.py) at
one match.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

KERNELS = ['k_cost_net_w24b', 'k_cost_net_w24b_rerun']       # (ahead of the next import: tests/test_cost_f24_cpu.py takes the list from here)

from test_cost_f24_cpu import random_layers  # noqa: E402
from test_cyl_code_object_cpu import ROOT, code_object, kernel_meta, kernel_text, loops  # noqa: E402, F401  (code_object: the module's fixture)


@pytest.mark.parametrize('name', KERNELS)
def test_resources(code_object, name):
    """No scratch, no spills, both register kinds together within 256 (two workgroups per CU), no LDS beside the dynamic buffer of CV_BUF
    floats."""
    asm, notes = code_object
    m = kernel_meta(notes, name)
    print(name, m)
    assert m['private_segment_fixed_size'] == 0, 'scratch memory'
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    assert m['vgpr_count'] <= 256 and m['agpr_count'] <= 256          # .vgpr_count of the unified file counts both kinds
    assert m['group_segment_fixed_size'] == 0, 'static LDS beside the dynamic buffer'
    src = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'costnet.hip')).read()
    cv_buf = int(re.search(r'#define CV_BUF (\d+)', src).group(1))
    w24b = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'costnet_w24b.hip')).read()
    launch = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'cnn_launch.hip')).read()      # (the cost kernels' one launcher)
    assert launch.count('size_t lds = sizeof(float) * CV_BUF;') == 1 and 2 * 4 * cv_buf <= 160 * 1024
    # layer 1's resident plane: in front of the layer-0 maps, even strides, the bank plan of the file's head
    rs, cs = (int(re.search(rf'#define {n} (\d+)', w24b).group(1)) for n in ('CWB_RS1', 'CWB_CS1'))
    sm = int(re.search(r'#define CVA_SM (\d+)', src).group(1))
    assert rs % 2 == 0 and cs % 2 == 0 and 32 * cs <= sm and 17 * rs + 18 <= cs
    banks = sorted(((lk * cs + 2 * ty * rs + 4 * tx + wd) % 64) for lk in range(2) for ty in range(4) for tx in range(4) for wd in range(2))
    assert banks == list(range(64)), 'a half-wave (16 windows x 2 channels) of one ds_read_b64 takes every bank once'
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
    """Static count per k-loop, four k-steps per iteration.  Every loop of W24_LOOPS (tests/test_cost_f24_cpu.py) and, once each:
    * layer 1 on F(2x4) tiles (one runtime loop over the three planes around one round): four pass loops of 6 x 2 x 4 = 48;
    * layer 3's F(2x4) round: four pass loops of 48;
    * layer 3's F(2x2) tail (a pair over the one M-tile of tile rows 4, 5): four loops of 4 x 2 x 4 = 32."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    counts = [c for c in counts if c]
    print(f'MFMAs per k-loop of {name}:', counts)
    assert counts == [8] * 2 + [16] * 13 + [32] * 24 + [48] * 17 + [64] * 12, counts
    total = sum(1 for _, op, _ in text if op.startswith('v_mfma'))
    assert total - sum(counts) == (30 + 18) * 4 * 2


@pytest.mark.parametrize('name', KERNELS)
def test_the_f24_pass_loops(code_object, name):
    """The sixteen F(2x4) pass loops (layers 1, 2, 3, 4): per iteration four k-steps of two window rows of six words (24 ds_read_b64) and 48
    MFMAs, no copies between the register files."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    hit = []
    for a, b in loops(text):
        ops = [op for _, op, _ in text[a:b + 1]]
        if sum(1 for o in ops if o.startswith('v_mfma')) == 48 and ops.count('ds_read_b64') == 24:
            hit.append(sum(1 for o in ops if o.startswith('v_accvgpr')))
    assert hit == [0] * 16, hit


def test_one_kernel_pair_and_one_launch_path(code_object):
    """The fp32 cost net is one kernel and its masked twin: beside them only the split form's kernels (k_cost_net_h3...) begin with
    k_cost_net in the gfx950 code object.  Their host side is plain functions over one parameter struct: nothing in the cost-net half of
    csrc/cnn_launch.hip is a template."""
    asm, _ = code_object
    names = {s[:int(n)] for n, s in re.findall(r'^[0-9a-f]+ <_Z(\d+)(k_cost_net\w*)>:$', asm, flags=re.M)}      # _Z<length><name><arguments>
    print(sorted(names))
    assert {n for n in names if not n.startswith('k_cost_net_h3')} == set(KERNELS)
    assert any(n.startswith('k_cost_net_h3') for n in names), 'the split form went missing: the pattern no longer finds kernels?'
    launch = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'cnn_launch.hip')).read()
    head, mark, cost = launch.partition('// ---- cost net ----')
    assert mark and 'cost_net_launch' in cost and 'buf_cost_volume_net_w24b_gather' in cost
    assert 'template' not in cost


def test_issued_count_per_match():
    """26 608 -> 24 048 issued matrix instructions per match (four wavefronts), from the layer shapes."""
    # layer 1: 96 input channels = 24 k-steps, 64 outputs = 4 N-tiles; 8 x 8 F(2x2) tiles = 4 M-tiles x 16 | 8 x 4 F(2x4) tiles = 2 M-tiles x 24
    l1_old, l1_new = 4 * 16 * 4 * 24, 2 * 24 * 4 * 24
    assert (l1_old, l1_new) == (6144, 4608) and 8 * 4 == 2 * 16
    # layer 3: 64 input channels = 16 k-steps, 128 outputs = 8 N-tiles; 3 M-tiles x 16 | one M-tile x 24 (5 x 3 tiles) + one M-tile x 16
    l3_old, l3_new = 3 * 16 * 8 * 16, (24 + 16) * 8 * 16
    assert (l3_old, l3_new) == (6144, 5120) and 5 * 3 <= 16
    assert 26608 - (l1_old - l1_new) - (l3_old - l3_new) == 24048
    # per wavefront of layer 1: a pair over one M-tile, three planes of 8 k-steps
    assert 2 * 24 * 8 * 3 == 1152 == l1_new // 4


def test_filter_sets_and_form_argument():
    """The two sets are buf_winograd_f24_tile_weights of the sliced filters and live in buffers of their own; a part that is not selected
    passes a null pointer; f24= keeps its values and meaning; a net with an explicit f24= and no f24b= is the net it was."""
    from buffer_amd import _lib, ops
    L = _lib.lib()
    layers = random_layers(3)
    assert ops.COST_F24_DEFAULT == 'all' and ops.COST_F24B_DEFAULT in ops.COST_F24B_PARTS
    want = {'all': (1, 3), 'l1': (1,), 'l3': (3,), 'off': ()}
    off = ops.CostVolumeNet(layers, 'cpu', f24b='off')
    assert off.parts == (2, 4, 6) and off.parts_b == () and [bool(p) for p in off._fpb] == [True] * 3 + [False] * 2
    for part, ls in want.items():
        net = ops.CostVolumeNet(layers, 'cpu', f24b=part)
        assert net.parts == (2, 4, 6) and net.parts_b == ls and len(net.wt24) == 3 and len(net._fp) == 3
        assert [t is not None for t in net.wt24b] == [l in ls for l in (1, 3)] == [bool(p) for p in net._fpb[3:]]
        assert [p for p in net._fpb[:3]] == [p for p in net._fp]
        for a, b in zip(net.wt + net.wt24, off.wt + off.wt24):
            assert np.array_equal(a.numpy(), b.numpy())
        for l, t in zip((1, 3), net.wt24b):
            if t is None:
                continue
            w = layers[l][0]
            w2d = np.ascontiguousarray(np.transpose(w, (0, 3, 1, 2, 4)).reshape(64, 96, 3, 3)) if l == 1 else np.ascontiguousarray(w[:, :, :, 0, :])
            cout, cin = w2d.shape[:2]
            ref = np.empty(24 * cout * cin, np.float32)
            assert L.buf_winograd_f24_tile_weights(w2d.ctypes.data, cout, cin, ref.ctypes.data) == 0
            assert t.numel() == ref.size and np.array_equal(t.numpy(), ref)
            assert all(t.data_ptr() != u.data_ptr() for u in net.wt + [x for x in net.wt24 if x is not None])
    assert ops.CostVolumeNet(layers, 'cpu').parts_b == want[ops.COST_F24B_DEFAULT] and ops.CostVolumeNet(layers, 'cpu').parts == (2, 4, 6)
    for f24 in ('all', 'l2', 'l4', 'l6', 'off', True, False):          # an explicit f24= alone: the older kernels, as they were
        assert ops.CostVolumeNet(layers, 'cpu', f24=f24).parts_b == ()
    mixed = ops.CostVolumeNet(layers, 'cpu', f24='l4', f24b='l3')
    assert mixed.parts == (4,) and mixed.parts_b == (3,) and [bool(p) for p in mixed._fpb] == [False, True, False, False, True]
    assert ops.CostVolumeNet(layers, 'cpu', f24b=True).parts_b == (1, 3) and ops.CostVolumeNet(layers, 'cpu', f24b=False).parts_b == ()
    split = ops.CostVolumeNetSplit(layers, 'cpu', f24b='l1')
    assert split.parts_b == (1,) and (not split.safe or split.f32.parts_b == (1,))
    assert ops.CostVolumeNetSplit(layers, 'cpu', f24='all').parts_b == ()
    for bad in ('l2', 'some', 1):
        with pytest.raises(ValueError):
            ops.CostVolumeNet(layers, 'cpu', f24b=bad)
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
    sets = (C.c_void_p * 5)()
    assert L.buf_cost_volume_net_w24b(x, x, 0, ten, ten, sets, x, None) == 0
    assert L.buf_cost_volume_net_w24b(None, None, 0, None, None, None, None, None) == 0
    assert L.buf_cost_volume_net_w24b(x, x, -1, ten, ten, sets, x, None) == -1 and b'm=-1' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24b(x, x, 2, ten, ten, None, x, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24b(x, None, 2, ten, ten, sets, x, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24b(x, x, 2, (C.c_void_p * 10)(), ten, sets, x, None) == -1 and b'null weights for layer 0' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24b_gather(x, 7, x, x, 0, ten, ten, sets, x, None) == 0
    assert L.buf_cost_volume_net_w24b_gather(x, 6, x, x, 2, ten, ten, sets, x, None) == -1 and b'ele_n=6' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24b_gather(x, 7, x, x, 2, ten, ten, None, x, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_w24b_gather(x, 7, None, x, 2, ten, ten, sets, x, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_split_safe_w24b(x, x, 7, None, None, 0, eleven, ten, ten, ten, sets, x, None, x, None) == 0
    assert L.buf_cost_volume_net_split_safe_w24b(x, x, 7, None, None, -2, eleven, ten, ten, ten, sets, x, None, x, None) == -1
    assert b'm=-2' in L.buf_last_error()
    assert L.buf_cost_volume_net_split_safe_w24b(x, x, 7, None, None, 2, eleven, ten, ten, ten, None, x, None, x, None) == -1
    assert b'null argument' in L.buf_last_error()
    assert L.buf_cost_volume_net_split_safe_w24b(x, x, 7, x, None, 2, eleven, ten, ten, ten, sets, x, None, x, None) == -1
    assert b'one row list without the other' in L.buf_last_error()
    assert L.buf_cost_volume_net_split_safe_w24b(x, x, 6, x, x, 2, eleven, ten, ten, ten, sets, x, None, x, None) == -1
    assert b'ele_n=6' in L.buf_last_error()


def test_restatement_meets_its_bound_at_one_match():
    """tools/cost_f24b_restate.py, the float32 restatement the kernel was written from: at the first match of tests/golden/match_tiny.npz
    the new forms stay below 1e-4 of the network in float64 (ind in [0, 20)) -- the bound of the kernel's GPU tests.  (Over all 40 matches
    and 70 random maps: profiles/cost_f24b_ab.md.)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import cost_f24b_restate as rb
    finally:
        sys.path.pop(0)
    layers = rb.r.released_layers()
    se, te = rb.r.golden_matches()
    ref = rb.ind_of(se[0], te[0], layers, 'f64')
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'match_tiny.npz'))['ind'][0]
    assert abs(ref - gold) <= 1e-4 * max(1.0, abs(gold)) + 2e-4
    for form in rb.FORMS:
        e = abs(rb.ind_of(se[0], te[0], layers, form) - ref)
        print(f'restatement, form {form}: |ind - ind64| = {e:.2e}')
        assert e < 1e-4
