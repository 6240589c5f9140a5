"""k_cyl_net_w25t (csrc/convnet_w25t.hip): the fused kernel with, in the layers of 128 output channels, the direct round of output row 6 on
taps the host formed (the filter rows 0 and 1 as they are) and in front of the Winograd round.  The reference is the float64 stack (torch
on the CPU); the metric is the largest error over the output scale of the whole map, stated for the whole map and for row 6 alone, each
beside the figure of the parent form (row6='off') on the same input.  Bounds: 1e-5 against float64 (that of
tests/test_cyl_f25_gpu.py), and row 6 no worse than twice the parent's figure (the 2 x rule of profiles/f25_ab.md).

The taps are another rounding of row 6 (exact filter values instead of differences of rounded Winograd blocks), so the new kernel is
not bit-equal to the parent; where it must be -- no tap set and the old order, the order alone (the same arithmetic in another
sequence), taps that are all zero -- the comparisons are bit for bit.

Measured on the MI355X (max over the cases of this file, error over the output scale): whole map 2.42e-06 (the parent kernel on the same
inputs 2.62e-06), row 6 1.51e-06 (parent 1.64e-06); the largest ratio of a row-6 figure to the parent's is 1.46."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cyl_bottom_row_gpu import errors, stack64
from test_cyl_f24a_gpu import STACK_B, random_layers, single_tap

pytestmark = pytest.mark.gpu
BOUND = 1e-5
WIDE_B = [1, 2]                  # stack B's layers with 128 output channels: 64 -> 128, 128 -> 128


def bits(t):
    return t.contiguous().view(torch.int32)


def nets_of(layers, dev):
    """[taps and order, the parent kernel]"""
    from buffer_amd import ops
    wide = [l for l, (w, _, _) in enumerate(layers) if w.shape[0] == 128]
    new = ops.CylindricalNet(layers, dev, row6='both')
    old = ops.CylindricalNet(layers, dev, row6='off')
    assert new.taps_layers == wide and new.row6_first and new.fn == 'buf_cylindrical_net_w25t'
    assert old.taps_layers == [] and not old.row6_first and old.fn == 'buf_cylindrical_net_w25'
    return [new, old]


def check(name, x, layers, nets, dev):
    """the new kernel and the parent against float64; returns the new kernel's output"""
    h = stack64(x.cpu(), layers, 'cpu').to(dev)
    y, yp = nets[0](x), nets[1](x)
    e_all, e6, _, scale = errors(y, h)
    p_all, p6, _, _ = errors(yp, h)
    print(f'{name}: scale {scale:.3e} | whole map {e_all:.2e} (parent {p_all:.2e}) | row 6 {e6:.2e} (parent {p6:.2e})')
    assert e_all <= BOUND and e6 <= BOUND
    assert e6 <= 2 * p6, (e6, p6)
    return y


@pytest.fixture(scope="module")
def released(dev):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    pe = PatchEmbedder(load_weights("3dmatch"), dev, THREEDMATCH)
    nets = nets_of(pe.layers, dev)
    assert nets[0].taps_layers == [2, 3] and list(nets[0]._re) == [1, 5, 3, 3, 5, 5, 1, 0]
    return pe.layers, nets


@pytest.fixture(scope="module")
def dense70(released, dev):
    """signed / non-negative -> (x [70, 48, 140], the new kernel's output): computed once, shared, left unchanged"""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(2570)
    out = {}
    for signed in (True, False):
        x = torch.rand((70, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        out[signed] = (x, check(f'released, n = 70, signed={signed}', x, layers, nets, dev))
    return out


@pytest.fixture(scope="module")
def input_b(dev):
    g = torch.Generator(device='cpu').manual_seed(33)
    return (torch.rand((3, 16, 140), generator=g) * 2 - 1).to(dev)


def test_stack_b_is_a_stack_of_the_kernel():
    from buffer_amd import _lib
    ci, co = (C.c_int * 8)(*STACK_B[:-1]), (C.c_int * 8)(*STACK_B[1:])
    assert _lib.lib().buf_cylindrical_net_wg_supports(ci, co) == 0, _lib.lib().buf_last_error()
    assert [l for l in range(8) if STACK_B[l + 1] == 128] == WIDE_B


@pytest.mark.parametrize("signed", [True, False])
def test_released_weights_and_batch_order(released, dense70, dev, signed):
    """70 patches against float64; 1 and 3 patches give the first rows of 70 and a permuted batch the permuted result, bit for bit"""
    layers, nets = released
    x, y = dense70[signed]
    for n in (1, 3):
        yn = check(f'released, n = {n}, signed={signed}', x[:n], layers, nets, dev)
        assert torch.equal(bits(yn), bits(y[:n]))
    perm = torch.randperm(70, generator=torch.Generator(device='cpu').manual_seed(7)).to(dev)
    assert torch.equal(bits(nets[0](x[perm])), bits(y[perm]))


@pytest.mark.parametrize("n", [1, 3, 70])
def test_stack_b(dev, n):
    layers = random_layers(STACK_B)
    nets = nets_of(layers, dev)
    g = torch.Generator(device='cpu').manual_seed(250 + n)
    for signed in (True, False):
        x = torch.rand((n, 16, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'stack B, n = {n}, signed={signed}', x, layers, nets, dev)


@pytest.mark.parametrize("layer", WIDE_B + [5])
@pytest.mark.parametrize("tap", range(9))
def test_single_tap_filters(dev, input_b, layer, tap):
    """Each 128-output layer of stack B and its first 32-output layer (64 -> 32): the layer's output is a shifted copy of its input"""
    layers = single_tap(random_layers(STACK_B), layer, tap)
    check(f'layer {layer}, tap ({tap // 3}, {tap % 3})', input_b, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("b", range(3))
def test_taps_of_filter_row_2_leave_row_6_alone(dev, input_b, b):
    """Both 128-output layers with one tap in filter row 2.  Row 6 looks at the rows 5 and 6 through the filter rows 0 and 1 only: its tap
    sets are all zero, the direct rounds add exact zeros to the bias, and so do the parent's (its taps, U_0 and U_1 - U_2 of such a filter,
    are exact zeros as well).  Everything else is the parent's arithmetic: the two kernels agree bit for bit, and the float64 stack says
    that the tap still reaches the rows 0..5."""
    from buffer_amd import ops
    layers = random_layers(STACK_B)
    for l in WIDE_B:
        layers = single_tap(layers, l, 6 + b)
        assert not ops.cyl_row6_tile_taps(layers[l][0]).any()
    nets = nets_of(layers, dev)
    y = check(f'filter row 2, tap b = {b}', input_b, layers, nets, dev)
    assert torch.equal(bits(y), bits(nets[1](input_b)))
    zero = [(np.zeros_like(w) if l in WIDE_B else w, bb, r) for l, (w, bb, r) in enumerate(layers)]
    assert not torch.equal(y[:, :, :6], nets_of(zero, dev)[0](input_b)[:, :, :6])


MASKS = {'row 5 only': (slice(5, 6), slice(None)), 'row 6 only': (slice(6, 7), slice(None)), 'column 0 only': (slice(None), slice(0, 1)),
         'column 19 only': (slice(None), slice(19, 20)), 'columns 15 and 16 only': (slice(None), slice(15, 17))}


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_masked_inputs(released, dev, mask):
    """The azimuth wrap (columns 0 and 19) and the seam between the direct columns 0..15 and lane 15's tile (columns 15 and 16)"""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(len(mask))
    base = torch.rand((3, 48, 7, 20), generator=g) * 2 - 1
    x = torch.zeros_like(base)
    rows, cols = MASKS[mask]
    x[:, :, rows, cols] = base[:, :, rows, cols]
    check(mask, x.reshape(3, 48, 140).to(dev), layers, nets, dev)


@pytest.mark.parametrize("layer,channel", [(1, c) for c in (0, 3, 4, 63)] + [(2, c) for c in (0, 3, 4, 63, 64, 127)])
def test_one_input_channel_alone(dev, input_b, layer, channel):
    """The layer's filters are zero but for one input channel: the tiling of the taps by k-step and lane"""
    layers = random_layers(STACK_B)
    w, b, relu = layers[layer]
    keep = np.zeros_like(w)
    keep[:, channel] = w[:, channel] * 8                    # (one of Cin channels: scaled up to the size of the whole layer's sum)
    layers[layer] = (keep, b, relu)
    check(f'layer {layer}, input channel {channel} alone', input_b, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("layer", WIDE_B)
@pytest.mark.parametrize("channel", [0, 15, 16, 31, 32, 127])
def test_one_output_channel_alone(dev, input_b, layer, channel):
    """The layer's filters and biases are zero but for one output channel: the tiling of the taps by lane and N-tile"""
    layers = random_layers(STACK_B)
    w, b, relu = layers[layer]
    kw, kb = np.zeros_like(w), np.zeros_like(b)
    kw[channel], kb[channel] = w[channel] * 8, b[channel]
    layers[layer] = (kw, kb, relu)
    check(f'layer {layer}, output channel {channel} alone', input_b, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("layer", WIDE_B)
def test_zero_filters_and_a_random_bias(dev, input_b, layer):
    """The layer's output is relu(bias) at every position: a bias that more than one accumulator carries shows as a multiple"""
    layers = random_layers(STACK_B)
    w, b, relu = layers[layer]
    b = np.random.default_rng(5).standard_normal(b.shape).astype(np.float32)
    layers[layer] = (np.zeros_like(w), b, relu)
    check(f'layer {layer}, bias only', input_b, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("layer", WIDE_B)
def test_a_layer_without_relu(dev, input_b, layer):
    layers = random_layers(STACK_B)
    w, b, _ = layers[layer]
    layers[layer] = (w, b, False)
    check(f'layer {layer} without ReLU', input_b, layers, nets_of(layers, dev), dev)


def test_without_sets_and_in_the_old_order_bit_for_bit_k_cyl_net_w25(released, dense70, dev):
    """buf_cylindrical_net_w25t without a tap set and with order = 0 runs the layer forms of buf_cylindrical_net_w25 in every layer (both
    reach k_cyl_net_w25t: cyl_prepare hands it the same parameters)"""
    from buffer_amd import _lib, ops
    layers, nets = released
    old = nets[1]
    x = dense70[True][0][:67]
    y = torch.empty((67, 32, 7, 20), dtype=torch.float32, device=dev)
    none = (C.c_void_p * 8)()
    ops.check(_lib.lib().buf_cylindrical_net_w25t(ops._ptr(x), 67, old._wp, old._bp, old._ci, old._co, old._re, old._w24p, old._w25p, none, 0,
                                                  ops._ptr(y), ops._stream()), "buf_cylindrical_net_w25t")
    assert torch.equal(bits(y), bits(old(x)))


def test_the_parts_alone(released, dense70, dev):
    """Taps only and order only: each equals itself across repeated calls.  The order alone changes no arithmetic: the bits of row6='off';
    and with the taps the order changes nothing either."""
    from buffer_amd import ops
    layers, nets = released
    x, y = dense70[True]
    taps, order = ops.CylindricalNet(layers, dev, row6='taps'), ops.CylindricalNet(layers, dev, row6='order')
    assert taps.taps_layers == [2, 3] and not taps.row6_first and order.taps_layers == [] and order.row6_first
    assert taps.fn == order.fn == 'buf_cylindrical_net_w25t'
    yt, yo = taps(x), order(x)
    for _ in range(2):
        assert torch.equal(bits(taps(x)), bits(yt)) and torch.equal(bits(order(x)), bits(yo))
    assert torch.equal(bits(yo), bits(nets[1](x)))
    assert torch.equal(bits(yt), bits(y))
    check('taps only', x[:3], layers, [taps, nets[1]], dev)


def test_masked_rerun_takes_the_same_kernel(released, dev):
    """Through ops.CylindricalNetSplit the fp32 re-run of the flagged patches (an overflowing patch, a NaN) is k_cyl_net_w25t_rerun: the
    plain call's result on them, bit for bit; the other patches keep what the split kernel wrote."""
    from buffer_amd import ops
    layers, nets = released
    split, plain = ops.CylindricalNetSplit(layers, dev, row6='both'), ops.CylindricalNetSplit(layers, dev, row6='off')
    assert split.safe and split.taps_layers == [2, 3] and split.row6_first and split.fn == 'buf_cylindrical_net_split_safe_w25t'
    assert plain.fn == 'buf_cylindrical_net_split_safe_w25'
    g = torch.Generator(device='cpu').manual_seed(79)
    bad = torch.rand((23, 48, 140), generator=g).to(dev)
    bad[2] *= 1e6
    bad[22, 47, 139] = float('nan')
    y, y32, ys = split(bad), nets[0](bad), plain(bad)
    rows = sorted(np.nonzero(split.last_flags.cpu().numpy())[0].tolist())
    assert rows == [2, 22]
    rr = torch.tensor(rows, device=dev)
    keep = torch.tensor([r for r in range(23) if r not in rows], device=dev)
    assert torch.equal(bits(y[rr]), bits(y32[rr]))                      # bitwise, NaN patterns included
    assert torch.equal(bits(y[keep]), bits(ys[keep]))


def test_no_patches(released, dev):
    from buffer_amd import ops
    layers, nets = released
    y = nets[0](torch.empty((0, 48, 140), device=dev))
    assert y.shape == (0, 32, 7, 20)
    assert ops.CylindricalNetSplit(layers, dev, row6='both')(torch.empty((0, 48, 140), device=dev)).shape == (0, 32, 7, 20)
