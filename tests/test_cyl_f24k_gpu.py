"""k_cyl_net_w24k (csrc/convnet_w24k.hip): the descriptor CNN with F(2x4, 3x3) tiles in its 64-output layers of Cin % 64 == 0 as well
(two wavefronts per N-tile pair, each over half of K, partial sums exchanged through LDS), against the float64 torch stack under the
project's bound (1e-5 of the output scale, on all rows and on row 6 separately: fp32 accumulation over K <= 9 x 128 products per output
leaves ~1e-7 x sqrt(K) of the scale per layer, eight layers; the CPU restatement of this arithmetic, tools/f24k_restate.py, measured
1.6e-6 at worst), and against the same filters in the two older forms (2e-5: the sum of the two bounds): F(2x4) in the 128-output layers
only (f24k=False) and F(2x2) throughout (k_cyl_net_wg, f24=False)."""
import numpy as np
import pytest
import torch

from test_cyl_bottom_row_gpu import errors, stack64

pytestmark = pytest.mark.gpu
BOUND = 1e-5
SECOND = [32, 128, 128, 64, 64, 32, 32, 32, 32]


@pytest.fixture(scope="module")
def released(dev):
    """(layers, [the product's net: flags 1 5 3 3 5 5 1 0, the bit-1-only net, the F(2x2) net])"""
    from buffer_amd import ops
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    pe = PatchEmbedder(load_weights("3dmatch"), dev, THREEDMATCH)
    assert pe.fused.entry == "buf_cylindrical_net_wg" and list(pe.fused._re) == [1, 5, 3, 3, 5, 5, 1, 0]
    w24 = ops.CylindricalNet(pe.layers, dev, f24k=False)
    assert list(w24._re) == [1, 1, 3, 3, 1, 1, 1, 0]
    return pe.layers, [pe.fused, w24, ops.CylindricalNet(pe.layers, dev, f24=False)]


def random_layers(seed=24):
    rng = np.random.default_rng(seed)
    layers = []
    for l in range(8):
        cin, cout = SECOND[l], SECOND[l + 1]
        w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)     # keeps the activations' scale
        b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        layers.append((w, b, l < 7))
    return layers


def nets_of(layers, dev):
    from buffer_amd import ops
    nets = [ops.CylindricalNet(layers, dev), ops.CylindricalNet(layers, dev, f24k=False), ops.CylindricalNet(layers, dev, f24=False)]
    assert [f & 4 for f in nets[0]._re] == [4 if (co == 64 and ci % 64 == 0) else 0 for ci, co in zip(nets[0].cin, nets[0].cout)]
    assert not any(f & 4 for f in nets[1]._re) and not any(f & 6 for f in nets[2]._re)
    return nets


@pytest.fixture(scope="module")
def second(dev):
    """Random filters, 32 -> 128 -> 128 -> 64 -> 64 -> 32 -> 32 -> 32 -> 32: flagged 64-output layers at Cin = 128 (two barriers around the
    exchange, four iterations of the k-loop per half) and at Cin = 64 (one barrier, two iterations)"""
    layers = random_layers()
    return layers, nets_of(layers, dev)


def check(name, x, layers, nets, dev):
    """the K-split net against float64 and against the two older forms; returns its output"""
    y, y24, y22 = (net(x) for net in nets)
    e_all, e6, e05, scale = errors(y, stack64(x, layers, dev))
    f24 = (y - y24).abs().max().item() / scale
    f22 = (y - y22).abs().max().item() / scale
    print(f'{name}: scale {scale:.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e} | vs f24k=False {f24:.2e} | vs f24=False {f22:.2e}')
    assert e6 < BOUND and e05 < BOUND and e_all < BOUND
    assert f24 < 2 * BOUND and f22 < 2 * BOUND
    return y


@pytest.mark.parametrize("channel", [0, 47])
def test_impulses_at_every_position(released, dev, channel):
    """Patch p holds a single 1.0 at map position p of one input channel.  This is also the case that shows the zero words of the
    channels 64..127 surviving the exchange: the released order is a flagged 64 -> 64 layer (exchange through the rows of those channels),
    then 64 -> 128, then 128 -> 128, whose window rows in the elevation padding read those words; the impulses of map rows 0 and 6
    (patches 0..19 and 120..139) put the non-zero activations next to that padding, and a word left non-zero would enter rows 0 and 6
    of layer 3's output in every patch."""
    layers, nets = released
    x = torch.zeros((140, 48, 140))
    x[torch.arange(140), channel, torch.arange(140)] = 1.0
    check(f'impulses in channel {channel}', x.to(dev), layers, nets, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_dense_inputs_and_batch_order(released, dev, n):
    """1, 3 and 513 patches (one more than a round of 256 CUs x 2 workgroup slots), signed and non-negative; a permuted batch gives the
    permuted result bit for bit."""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(2400 + n)
    for signed in (True, False):
        x = torch.rand((n, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        y = check(f'n = {n}, {"signed" if signed else "non-negative"}', x, layers, nets, dev)
        perm = torch.randperm(n, generator=g).to(dev)
        assert torch.equal(nets[0](x[perm]), y[perm])


def test_rows_0_and_6_only(released, dev):
    """Non-zero input in map rows 0 and 6 only, dense along the azimuth: the rows whose windows reach into the elevation padding."""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(6)
    x = torch.zeros((5, 48, 7, 20))
    x[:, :, [0, 6]] = torch.rand((5, 48, 2, 20), generator=g) * 2 - 1
    check('rows 0 and 6 only', x.reshape(5, 48, 140).to(dev), layers, nets, dev)


def test_second_stack(second, dev):
    layers, nets = second
    g = torch.Generator(device='cpu').manual_seed(9)
    for signed in (True, False):
        x = torch.rand((37, 32, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'second stack, signed={signed}', x, layers, nets, dev)


@pytest.mark.parametrize("layer", [2, 3])
@pytest.mark.parametrize("fault", ["lower K half zero", "upper K half zero", "bias only"])
def test_k_halves_and_bias_made_gross(dev, layer, fault):
    """One flagged layer of the second stack (2: 128 -> 64, 3: 64 -> 64) with filters that are zero on the input channels of one K half --
    a half that is dropped, read from the wrong channels or added twice changes the whole output -- and with all-zero filters and a random
    bias: the layer's output is relu(bias), a bias that both halves carry shows doubled."""
    layers = random_layers()
    w, b, relu = layers[layer]
    w = w.copy()
    cin = w.shape[1]
    if fault == "lower K half zero":
        w[:, :cin // 2] = 0
    elif fault == "upper K half zero":
        w[:, cin // 2:] = 0
    else:
        w[:] = 0
        b = np.random.default_rng(5).standard_normal(b.shape).astype(np.float32)
    layers[layer] = (w, b, relu)
    nets = nets_of(layers, dev)
    assert nets[0]._re[layer] & 4
    g = torch.Generator(device='cpu').manual_seed(31)
    x = (torch.rand((9, 32, 140), generator=g) * 2 - 1).to(dev)
    check(f'layer {layer}, {fault}', x, layers, nets, dev)


def test_the_bit_1_kernel_stays_exercised(released, dev):
    """A stack with bit 1 only (f24k=False: F(2x4) in the 128-output layers alone) on its own against float64: the product no longer runs it."""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(12)
    x = (torch.rand((67, 48, 140), generator=g) * 2 - 1).to(dev)
    e_all, e6, e05, scale = errors(nets[1](x), stack64(x, layers, dev))
    print(f'bit 1 only: scale {scale:.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e}')
    assert e6 < BOUND and e05 < BOUND and e_all < BOUND


def test_masked_rerun_takes_the_k_split_kernel(released, dev):
    """ops.CylindricalNetSplit hands the fp32 re-run the flagged filter sets with bit 2: on the patches the split kernel flags the result is
    the plain call's (k_cyl_net_w24k), bit for bit."""
    from buffer_amd import ops
    layers, nets = released
    split = ops.CylindricalNetSplit(layers, dev)
    assert split.safe and list(split._re_safe) == [1, 5, 3, 3, 5, 5, 1, 0]
    g = torch.Generator(device='cpu').manual_seed(78)
    bad = torch.rand((23, 48, 140), generator=g).to(dev)
    bad[2] *= 1e6
    bad[22, 47, 139] = float('nan')
    y, y32 = split(bad), nets[0](bad)
    rows = sorted(np.nonzero(split.last_flags.cpu().numpy())[0].tolist())
    assert rows == [2, 22]
    rr = torch.tensor(rows, device=dev)
    assert torch.equal(y[rr].view(torch.int32), y32[rr].view(torch.int32))            # bitwise, NaN patterns included
