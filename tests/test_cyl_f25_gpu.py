"""The F(2x5) layer forms (csrc/convnet_w25.hip): the descriptor CNN with F(2x5, 3x3) tiles -- 2 rows x 5 azimuth columns, 4 x 4 regular tiles
for the 7 x 20 map, no direct round of row 6 -- in the 64- and 32-output layers.  Each comparison has two bounds: against the float64
torch stack 1e-5 of the output scale, on the whole map and on row 6 alone (the CPU restatement of this summation order,
tools/f25_restate.py, measured 1.5e-6 at worst), and against the same filters in the older forms 2e-5, the sum of two bounds:
F(2x4) tiles in every layer (f24a='all', f25='off') and F(2x2) throughout (k_cyl_net_wg, f24=False).

Stack A puts a 32-output layer directly in front of a wider one, which the F(2x2) forms reject (tests/test_cyl_f24a_gpu.py): its
references are the float64 stack and the F(2x4) forms.  The impulses put a single 1.0 at every map position: a wrong halo word, a wrong
padding factor of the rows -1, 7 and 8, or a wrong window at the edges tx = 3 / ty = 3 shows there as an error of the order of a filter
tap.

Measured on the MI355X (max over the cases, error over the output scale): against float64 2.3e-06 on the whole map, 1.4e-06 on row 6;
against the older kernels 3.3e-06."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cyl_bottom_row_gpu import errors, stack64
from test_cyl_f24a_gpu import STACK_A, STACK_B, random_layers, single_tap

pytestmark = pytest.mark.gpu
BOUND = 1e-5
RELEASED_F25 = [0, 1, 4, 5, 6, 7]


def nets_of(layers, dev, older=True):
    """[F(2x5) in the 64- and 32-output layers, F(2x4) in every layer, F(2x2)]; older = False: without the last"""
    from buffer_amd import ops
    new = ops.CylindricalNet(layers, dev, f25='all')
    assert new.f25_layers == [l for l, (w, _, _) in enumerate(layers) if w.shape[0] in (32, 64)]
    nets = [new, ops.CylindricalNet(layers, dev, f24a='all', f25='off')]
    assert nets[1].f25_layers == [] and nets[1].f24_all
    if older:
        nets.append(ops.CylindricalNet(layers, dev, f24=False))
        assert not nets[2].f24_layers and not nets[2].f25_layers
    return nets


@pytest.fixture(scope="module")
def released(dev):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    pe = PatchEmbedder(load_weights("3dmatch"), dev, THREEDMATCH)
    nets = nets_of(pe.layers, dev)
    assert nets[0].f25_layers == RELEASED_F25 and list(nets[0]._re) == [1, 5, 3, 3, 5, 5, 1, 0]
    return pe.layers, nets


@pytest.fixture(scope="module")
def stack_a(dev):
    layers = random_layers(STACK_A)
    return layers, nets_of(layers, dev, older=False)


@pytest.fixture(scope="module")
def stack_b(dev):
    layers = random_layers(STACK_B)
    return layers, nets_of(layers, dev)


@pytest.fixture(scope="module")
def input_b(dev):
    g = torch.Generator(device='cpu').manual_seed(31)
    return (torch.rand((9, 16, 140), generator=g) * 2 - 1).to(dev)


def check(name, x, layers, nets, dev):
    """the first net against float64 and against the others; returns its output"""
    ys = [net(x) for net in nets]
    e_all, e6, e05, scale = errors(ys[0], stack64(x, layers, dev))
    others = [(ys[0] - y).abs().max().item() / scale for y in ys[1:]]
    print(f'{name}: scale {scale:.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e} | vs the other forms ' + ' '.join(f'{o:.2e}' for o in others))
    assert e6 <= BOUND and e05 <= BOUND and e_all <= BOUND
    assert all(o <= 2 * BOUND for o in others)
    return ys[0]


@pytest.mark.parametrize("channel", [0, 47])
def test_impulses_at_every_position(released, dev, channel):
    """Patch p holds a single 1.0 at map position p of one input channel; channel 47 is the last of layer 0's third k-loop iteration."""
    layers, nets = released
    x = torch.zeros((140, 48, 140))
    x[torch.arange(140), channel, torch.arange(140)] = 1.0
    check(f'impulses in channel {channel}', x.to(dev), layers, nets, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_dense_inputs_and_batch_order(released, dev, n):
    """1, 3 and 513 patches (one more than the 512 workgroups a launch holds at once), signed and non-negative; a permuted batch gives
    the permuted result bit for bit."""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(2500 + n)
    for signed in (True, False):
        x = torch.rand((n, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        y = check(f'n = {n}, {"signed" if signed else "non-negative"}', x, layers, nets, dev)
        perm = torch.randperm(n, generator=g).to(dev)
        assert torch.equal(nets[0](x[perm]), y[perm])


@pytest.mark.parametrize("n", [1, 3, 513])
def test_stack_a(stack_a, dev, n):
    layers, nets = stack_a
    g = torch.Generator(device='cpu').manual_seed(170 + n)
    for signed in (True, False):
        x = torch.rand((n, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'stack A, n = {n}, signed={signed}', x, layers, nets, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_stack_b(stack_b, dev, n):
    layers, nets = stack_b
    g = torch.Generator(device='cpu').manual_seed(190 + n)
    for signed in (True, False):
        x = torch.rand((n, 16, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'stack B, n = {n}, signed={signed}', x, layers, nets, dev)


@pytest.mark.parametrize("part", ['out64', 'out32'])
def test_the_parts_alone(released, dev, part):
    """F(2x5) in the layers of one output width only, the others on F(2x4) tiles: the two forms next to each other in one stack"""
    from buffer_amd import ops
    layers, nets = released
    net = ops.CylindricalNet(layers, dev, f25=part)
    assert net.f25_layers == ([0, 1, 4, 5] if part == 'out64' else [6, 7])
    g = torch.Generator(device='cpu').manual_seed(66)
    x = (torch.rand((5, 48, 140), generator=g) * 2 - 1).to(dev)
    check(f'f25 = {part}', x, layers, [net] + nets[1:], dev)


@pytest.mark.parametrize("layer", [0, 5])
@pytest.mark.parametrize("tap", range(9))
def test_single_tap_filters(dev, input_b, layer, tap):
    """Stack B's layer 0 (16 -> 64) and its first 32-output layer (64 -> 32): the layer's output is a shifted copy of its input"""
    layers = single_tap(random_layers(STACK_B), layer, tap)
    check(f'layer {layer}, tap ({tap // 3}, {tap % 3})', input_b, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("layer", [0, 5])
def test_zero_filters_and_a_random_bias(dev, input_b, layer):
    """The layer's output is relu(bias) at every position: a bias that more than one row or column component carries shows as a multiple."""
    layers = random_layers(STACK_B)
    w, b, relu = layers[layer]
    b = np.random.default_rng(5).standard_normal(b.shape).astype(np.float32)
    layers[layer] = (np.zeros_like(w), b, relu)
    check(f'layer {layer}, bias only', input_b, layers, nets_of(layers, dev), dev)


def test_without_a_set_bit_for_bit_k_cyl_net_w24a(released, dev):
    """buf_cylindrical_net_w25 without a single F(2x5) set runs the layer forms of buf_cylindrical_net_wg_all in every layer: bit for bit that
    entry point's output (both reach k_cyl_net_w25t: cyl_prepare hands it the same parameters)"""
    from buffer_amd import _lib, ops
    layers, nets = released
    old = nets[1]
    g = torch.Generator(device='cpu').manual_seed(41)
    x = (torch.rand((67, 48, 140), generator=g) * 2 - 1).to(dev)
    y = torch.empty((67, 32, 7, 20), dtype=torch.float32, device=dev)
    none = (C.c_void_p * 8)()
    ops.check(_lib.lib().buf_cylindrical_net_w25(ops._ptr(x), 67, old._wp, old._bp, old._ci, old._co, old._re, old._w24p, none, ops._ptr(y), ops._stream()),
              "buf_cylindrical_net_w25")
    assert torch.equal(y.view(torch.int32), old(x).view(torch.int32))


def test_masked_rerun_takes_the_same_kernel(released, dev):
    """Through ops.CylindricalNetSplit the fp32 re-run of the flagged patches (an overflowing patch, a NaN) is k_cyl_net_w25t_rerun: the
    plain call's result, bit for bit -- non-finite values included, which the padding factor of the rows outside the map turns into NaN
    in both alike."""
    from buffer_amd import ops
    layers, nets = released
    split = ops.CylindricalNetSplit(layers, dev, f25='all')
    assert split.safe and split.f25_layers == RELEASED_F25 and list(split._re_safe) == [1, 5, 3, 3, 5, 5, 1, 0]
    g = torch.Generator(device='cpu').manual_seed(78)
    bad = torch.rand((23, 48, 140), generator=g).to(dev)
    bad[2] *= 1e6
    bad[22, 47, 139] = float('nan')
    y, y32 = split(bad), nets[0](bad)
    rows = sorted(np.nonzero(split.last_flags.cpu().numpy())[0].tolist())
    assert rows == [2, 22]
    rr = torch.tensor(rows, device=dev)
    assert torch.equal(y[rr].view(torch.int32), y32[rr].view(torch.int32))            # bitwise, NaN patterns included
