"""The pass-split form (w24p_layer_psplit, csrc/convnet_w24p.hip): the flagged 64-output layers of the descriptor CNN in the pass-split form -- wavefront w owns
row component w of the F(2,3) row transform for all four N-tiles over the whole K, folds once, and wavefront q finishes N-tile q from
three received partial outputs.  Against the float64 torch stack under the project's bound (1e-5 of the output scale: the CPU restatement
of this summation order, tools/f24p_restate.py, measured 1.6e-6 at worst) and against the same filters in the older forms (2e-5, the sum
of two bounds): the K split (k_cyl_net_w24k, f24p=False) and F(2x2) throughout (k_cyl_net_wg, f24=False)."""
import numpy as np
import pytest
import torch

from test_cyl_bottom_row_gpu import errors, stack64

pytestmark = pytest.mark.gpu
BOUND = 1e-5
SECOND = [32, 64, 128, 128, 64, 64, 32, 32, 32]          # flagged: layer 3 (128 -> 64) and layer 4 (64 -> 64)
FLAGGED = {3: (128, 64), 4: (64, 64)}


def nets_of(layers, dev):
    """[pass split, K split, F(2x2)]"""
    from buffer_amd import ops
    nets = [ops.CylindricalNet(layers, dev, f24p=True), ops.CylindricalNet(layers, dev, f24p=False), ops.CylindricalNet(layers, dev, f24=False)]
    assert (nets[0].form, nets[1].form) == (1, 0) and list(nets[0]._re) == list(nets[1]._re)
    assert [f & 4 for f in nets[0]._re] == [4 if (co == 64 and ci % 64 == 0) else 0 for ci, co in zip(nets[0].cin, nets[0].cout)]
    return nets


@pytest.fixture(scope="module")
def released(dev):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    pe = PatchEmbedder(load_weights("3dmatch"), dev, THREEDMATCH)
    nets = nets_of(pe.layers, dev)
    assert list(nets[0]._re) == [1, 5, 3, 3, 5, 5, 1, 0]
    return pe.layers, nets


def random_layers(seed=24):
    rng = np.random.default_rng(seed)
    layers = []
    for l in range(8):
        cin, cout = SECOND[l], SECOND[l + 1]
        w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)     # keeps the activations' scale
        layers.append((w, (rng.standard_normal(cout) * 0.1).astype(np.float32), l < 7))
    assert all(layers[l][0].shape[:2] == (co, ci) for l, (ci, co) in FLAGGED.items())
    return layers


@pytest.fixture(scope="module")
def second(dev):
    layers = random_layers()
    return layers, nets_of(layers, dev)


@pytest.fixture(scope="module")
def second_input(dev):
    g = torch.Generator(device='cpu').manual_seed(31)
    return (torch.rand((9, 32, 140), generator=g) * 2 - 1).to(dev)


def check(name, x, layers, nets, dev):
    """the pass-split net against float64 and against the two older forms; returns its output"""
    y, yk, y22 = (net(x) for net in nets)
    e_all, e6, e05, scale = errors(y, stack64(x, layers, dev))
    fk = (y - yk).abs().max().item() / scale
    f22 = (y - y22).abs().max().item() / scale
    print(f'{name}: scale {scale:.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e} | vs f24p=False {fk:.2e} | vs f24=False {f22:.2e}')
    assert e6 < BOUND and e05 < BOUND and e_all < BOUND
    assert fk < 2 * BOUND and f22 < 2 * BOUND
    return y


@pytest.mark.parametrize("channel", [0, 47])
def test_impulses_at_every_position(released, dev, channel):
    """Patch p holds a single 1.0 at map position p of one input channel.  Also the case that shows the zero words of the channels
    64..127 surviving the exchange (layer 1 uses those rows, layer 3 reads the words in its elevation padding)."""
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


def test_rows_0_and_6_only(released, dev):
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(6)
    x = torch.zeros((5, 48, 7, 20))
    x[:, :, [0, 6]] = torch.rand((5, 48, 2, 20), generator=g) * 2 - 1
    check('rows 0 and 6 only', x.reshape(5, 48, 140).to(dev), layers, nets, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_second_stack(second, dev, n):
    layers, nets = second
    g = torch.Generator(device='cpu').manual_seed(90 + n)
    for signed in (True, False):
        x = torch.rand((n, 32, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'second stack, n = {n}, signed={signed}', x, layers, nets, dev)


@pytest.mark.parametrize("layer", sorted(FLAGGED))
@pytest.mark.parametrize("tap", range(9))
def test_single_tap_filters(dev, second_input, layer, tap):
    """One flagged layer with a single tap at (a, b) and the identity over the channels (output o takes input o, and at Cin = 128 half
    of input 64 + o, so both K halves count): the layer's output is a shifted copy of its input, and a row component that enters with
    the wrong sign, from the wrong window row or into the wrong N-tile shows as a negated, shifted or permuted copy."""
    layers = random_layers()
    w, b, relu = layers[layer]
    w = np.zeros_like(w)
    o = np.arange(64)
    w[o, o, tap // 3, tap % 3] = 1.0
    if w.shape[1] == 128:
        w[o, 64 + o, tap // 3, tap % 3] = 0.5
    layers[layer] = (w, b, relu)
    check(f'layer {layer}, tap ({tap // 3}, {tap % 3})', second_input, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("layer", sorted(FLAGGED))
def test_zero_filters_and_a_random_bias(dev, second_input, layer):
    """The layer's output is relu(bias) at every position: a bias that more than one pass carries shows as a multiple."""
    layers = random_layers()
    w, b, relu = layers[layer]
    b = np.random.default_rng(5).standard_normal(b.shape).astype(np.float32)
    layers[layer] = (np.zeros_like(w), b, relu)
    check(f'layer {layer}, bias only', second_input, layers, nets_of(layers, dev), dev)


def test_masked_rerun_takes_the_same_form(released, dev):
    """Through ops.CylindricalNetSplit the fp32 re-run of the flagged patches (an overflowing patch, a NaN) is k_cyl_net_w25t_rerun: the
    plain call's result, bit for bit."""
    from buffer_amd import ops
    layers, nets = released
    split = ops.CylindricalNetSplit(layers, dev, f24p=True)
    assert split.safe and split.form == 1 and list(split._re_safe) == [1, 5, 3, 3, 5, 5, 1, 0]
    g = torch.Generator(device='cpu').manual_seed(78)
    bad = torch.rand((23, 48, 140), generator=g).to(dev)
    bad[2] *= 1e6
    bad[22, 47, 139] = float('nan')
    y, y32 = split(bad), nets[0](bad)
    rows = sorted(np.nonzero(split.last_flags.cpu().numpy())[0].tolist())
    assert rows == [2, 22]
    rr = torch.tensor(rows, device=dev)
    assert torch.equal(y[rr].view(torch.int32), y32[rr].view(torch.int32))            # bitwise, NaN patterns included
