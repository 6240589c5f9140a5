"""The 128-output layers' F(2x4) form (w24_layer_pair, csrc/convnet_w24.hip): the descriptor CNN with its 128-output layers in the Winograd F(2x4, 3x3) form, against the
float64 torch stack under the project's bound (1e-5 of the output scale: fp32 accumulation over K <= 9 x 128 products per output leaves
~1e-7 x sqrt(K) of the scale per layer, eight layers; the F(2x4) transforms measured 1.0e-6 on the CPU restatement), against the
F(2x2) kernel on the same inputs and weights (2e-5: the sum of the two bounds), and bit for bit under a batch permutation and in the masked
re-run of the split path."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cyl_bottom_row_gpu import errors, stack64

pytestmark = pytest.mark.gpu
BOUND = 1e-5


@pytest.fixture(scope="module")
def released(dev):
    """(layers, the product's net [F(2x4) in the 128-output layers], the same filters in the F(2x2) form throughout)"""
    from buffer_amd import ops
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    pe = PatchEmbedder(load_weights("3dmatch"), dev, THREEDMATCH)
    assert pe.fused.entry == "buf_cylindrical_net_wg" and [f & 2 for f in pe.fused._re] == [2 if c == 128 else 0 for c in pe.fused.cout]
    return pe.layers, pe.fused, ops.CylindricalNet(pe.layers, dev, f24=False)


@pytest.fixture(scope="module")
def second(dev):
    """Random filters, 32 -> 128 -> 128 -> 64 -> 64 -> 32 -> 32 -> 32 -> 32: a 128-output layer at Cin = 32 (two iterations of the k-loop,
    the shortest the width rules allow, and as layer 0: straight behind the input load) and at Cin = 128"""
    from buffer_amd import _lib, ops
    widths = [32, 128, 128, 64, 64, 32, 32, 32, 32]
    ci, co = (C.c_int * 8)(*widths[:-1]), (C.c_int * 8)(*widths[1:])
    assert _lib.lib().buf_cylindrical_net_wg_supports(ci, co) == 0
    rng = np.random.default_rng(24)
    layers = []
    for l in range(8):
        cin, cout = widths[l], widths[l + 1]
        w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)     # keeps the activations' scale
        b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        layers.append((w, b, l < 7))
    return layers, ops.CylindricalNet(layers, dev), ops.CylindricalNet(layers, dev, f24=False)


def check(name, x, layers, net, net22, dev):
    y, y22 = net(x), net22(x)
    e_all, e6, e05, scale = errors(y, stack64(x, layers, dev))
    form = (y - y22).abs().max().item() / scale
    print(f'{name}: scale {scale:.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e} | F(2x4) vs F(2x2) form {form:.2e}')
    assert e6 < BOUND and e05 < BOUND and e_all < BOUND
    assert form < 2 * BOUND
    return y


@pytest.mark.parametrize("channel", [0, 47])
def test_impulses_reach_every_tile_seam_and_halo(released, dev, channel):
    """Patch p holds a single 1.0 at map position p of one input channel (channel 47: the last k-step's last lane quarter): its response
    crosses the tile seams (columns 3|4, 7|8, 11|12, 15|16, 19|0; rows 5|6) and the halo copies of every layer around p."""
    layers, net, net22 = released
    x = torch.zeros((140, 48, 140))
    x[torch.arange(140), channel, torch.arange(140)] = 1.0
    check(f'impulses in channel {channel}', x.to(dev), layers, net, net22, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_dense_inputs_and_batch_order(released, dev, n):
    """1, 3 and 513 patches (one more than a round of 256 CUs x 2 workgroup slots), signed and non-negative; a permuted batch gives the
    permuted result bit for bit."""
    layers, net, net22 = released
    g = torch.Generator(device='cpu').manual_seed(240 + n)
    for signed in (True, False):
        x = torch.rand((n, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        y = check(f'n = {n}, {"signed" if signed else "non-negative"}', x, layers, net, net22, dev)
        perm = torch.randperm(n, generator=g).to(dev)
        assert torch.equal(net(x[perm]), y[perm])


def test_second_stack(second, dev):
    layers, net, net22 = second
    g = torch.Generator(device='cpu').manual_seed(9)
    for signed in (False, True):
        x = torch.rand((37, 32, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'second stack, signed={signed}', x, layers, net, net22, dev)
    x = torch.zeros((140, 32, 140))
    x[torch.arange(140), 31, torch.arange(140)] = 1.0
    check('second stack, impulses in channel 31', x.to(dev), layers, net, net22, dev)


def test_masked_rerun_of_the_split_path_is_the_plain_call(released, dev):
    """ops.CylindricalNetSplit hands the fp32 re-run the flagged filter sets: on the patches the split kernel flags (an input beyond the
    f16 range, a NaN, an infinity) the result is the plain flagged call's, bit for bit; the other patches are the split kernel's."""
    from buffer_amd import ops
    layers, net, _ = released
    split = ops.CylindricalNetSplit(layers, dev)
    assert split.safe and [f & 2 for f in split._re_safe] == [2 if c == 128 else 0 for c in split.cout]
    g = torch.Generator(device='cpu').manual_seed(77)
    x = torch.rand((41, 48, 140), generator=g).to(dev)
    clean = split(x)
    assert split.range_fallbacks() == 0
    bad = x.clone()
    bad[3] *= 1e6
    bad[18, 5, 77] = float('nan')
    bad[40, 0, 0] = float('inf')
    y, y32 = split(bad), net(bad)
    rows = sorted(np.nonzero(split.last_flags.cpu().numpy())[0].tolist())
    assert rows == [3, 18, 40]
    rr = torch.tensor(rows, device=dev)
    keep = torch.tensor([i for i in range(41) if i not in rows], device=dev)
    assert torch.equal(y[rr].view(torch.int32), y32[rr].view(torch.int32))            # bitwise, NaN patterns included
    assert torch.equal(y[keep], clean[keep])
    assert float(y32[3].abs().max()) > 65504.0 and bool(torch.isfinite(y[3]).all())   # an overflowing patch with a finite fp32 result
