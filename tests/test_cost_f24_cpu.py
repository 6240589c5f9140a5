"""Host side and code object of the layer forms the *_w24 entry points added to the cost net (csrc/costnet_w24.hip: F(2x4) tiles in layers 2
and 4, the Winograd F(2x2) form in layer 6), in the one kernel pair that holds every form (k_cost_net_w24b / k_cost_net_w24b_rerun,
csrc/costnet_body.hip): the k-loops these forms brought, read off the gfx950 code object of the in-tree library; the three extra filter
sets and the form argument of the ops classes; the argument checks of the entry points; and the float32 restatement of the arithmetic
(tools/cost_f24_restate.py) at one match.  No GPU needed.

The forms were added in two steps, each to a kernel of its own beside the one before.  The loop lists of the two retired kernels live on
as F22_LOOPS and W24_LOOPS: the fused kernel holds all of them, and each step added exactly its own loops (the fused kernel's register
and memory bounds, its sixteen F(2x4) pass loops and its whole list: tests/test_cost_f24b_cpu.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_cyl_code_object_cpu import ROOT, code_object, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)
from test_cyl_f24_code_object_cpu import beyond, mfma_per_loop

SHAPES = [(32, 32, 3, 3, 3), (64, 32, 3, 3, 3), (64, 64, 3, 1, 3), (128, 64, 3, 1, 3), (128, 128, 3, 1, 3), (64, 128, 3, 1, 3),
          (64, 64, 3, 1, 3), (32, 64, 3, 1, 3), (32, 32, 3, 1, 3), (20, 32, 2, 1, 2)]


def random_layers(seed=0):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal(s) * np.sqrt(2.0 / np.prod(s[1:]))).astype(np.float32), (0.1 * rng.standard_normal(s[0])).astype(np.float32))
            for s in SHAPES]


from test_cost_f24b_cpu import KERNELS  # noqa: E402  (behind random_layers, which that module takes from here)

# MFMAs per k-loop (four k-steps per iteration; the direct layers: one tap per iteration) of the retired k_cost_net, read off a build of
# the last commit that had it -- every layer in its first form:
# * phase A.2 (layer 1, four chunks, a pair over one M-tile): 16 loops of 32;
# * layers 2 and 4 in the F(2x2) form (a pair over two M-tiles): four loops each of 64;
# * layer 3 (a pair over two M-tiles, then over the third): four loops of 64 and four of 32;
# * layer 5 (one N-tile, one M-tile; position-major stores): four loops of 16;
# * layer 6 direct (three M-tiles, four channel groups per tap): one loop of 48; layers 7..9: 16, 8, 8.
F22_LOOPS = [8] * 2 + [16] * 5 + [32] * 20 + [48] + [64] * 12
# ... and of the retired k_cost_net_w24, which added:
# * layers 2 and 4 on F(2x4) tiles (cw24_layer -> w24_round): four pass loops each of 6 components x 2 N-tiles x 4 k-steps = 48;
# * layer 5 once more with channel-major stores: four loops of 16;
# * layer 6 in the Winograd form (cw_layer at one N-tile and one M-tile): four loops of 4 x 4 = 16.
W24_LOOPS = [8] * 2 + [16] * 13 + [32] * 20 + [48] * 9 + [64] * 12


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """Static count per k-loop.  Every layer form the kernel can be switched to is in it once: the loops of the first forms (F22_LOOPS),
    those the forms of csrc/costnet_w24.hip added (W24_LOOPS), and beyond them exactly the loops of csrc/costnet_w24b.hip -- layer 1 and
    layer 3 on F(2x4) tiles, four pass loops of 48 each, and layer 3's F(2x2) tail, four loops of 32.
    Outside the loops are only the two fully unrolled GEMMs of phase A.1, (30 + 18) groups x 4 k-steps x 2 N-tiles = 384
    (cv_gemm_static has no loop to be inside of)."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    counts = mfma_per_loop(text)
    print(f'MFMAs per k-loop of {name}:', counts)
    assert sum(F22_LOOPS) == 1552 and W24_LOOPS == [8] * 2 + [16] * 13 + [32] * 20 + [48] * 9 + [64] * 12
    assert beyond(W24_LOOPS, F22_LOOPS) == ([16] * 8 + [48] * 8, [])
    assert beyond(counts, W24_LOOPS) == ([32] * 4 + [48] * 8, []), counts
    total = sum(1 for _, op, _ in text if op.startswith('v_mfma'))
    assert total - sum(counts) == (30 + 18) * 4 * 2


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
    own, and a part that is not selected passes a null pointer: that layer runs its first form.  The ten existing buffers do not change."""
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
