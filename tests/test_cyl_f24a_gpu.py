"""The layer forms on F(2x4) sets of their own (csrc/convnet_w24a.hip): the descriptor CNN with F(2x4) tiles in every layer -- layer 0 (Cin = 48, and 16 in the second
stack) through the pass-split form of the 64-output layers, the 32-output layers through the pass split over one N-tile pair.  Each
comparison has two bounds: against the float64 torch stack 1e-5 of the output scale, whole map and row 6 separately (the CPU restatement
of this summation order, tools/f24a_restate.py, measured 1.2e-6 at worst), and against the same filters in the older forms 2e-5, the
sum of two bounds: the pass split in the flagged layers only (f24p=True) and F(2x2) throughout (k_cyl_net_wg, f24=False).

Stack A puts a 32-output layer directly in front of a wider one.  The older forms reject such widths (their 32-output form runs its
exchange over the zero words of the channels 64..95), which the test asserts.  So the ONLY independent reference for stack A is the float64
stack: the second net it is compared with (f24a='out32', the F(2x2) form in the 64-output layer 0) runs the same new code in the 32-output
layers and checks layer 0 alone.  Likewise no kernel here takes a Cin that is not a multiple of 16 (every k-loop runs four k-steps per
iteration) or the 72 outputs in front of it, so "a layer no new form takes" at Cin = 72 is a stack every net refuses in the same way.

Measured on the MI355X (max over the cases, error over the output scale): against float64 2.4e-06 on the whole map, 1.3e-06 on row 6;
against the older kernels 2.5e-06."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cyl_bottom_row_gpu import errors, stack64

pytestmark = pytest.mark.gpu
BOUND = 1e-5
STACK_A = [48, 64, 32, 32, 64, 64, 64, 32, 32]           # 32-output form: Cin = 64 (layer 1), Cin = 32 in front of a wider layer (layer 2), last (layer 7)
STACK_B = [16, 64, 128, 128, 64, 64, 32, 32, 32]         # layer 0 with one k-loop iteration; 64 -> 32 and two 32 -> 32 layers
RELEASED_NEW = [0, 6, 7]


def nets_of(layers, dev, older=True):
    """[F(2x4) in all layers, F(2x4) in the flagged layers only (f24p=True), F(2x2)], or with older = False [all layers, the 32-output layers only]"""
    from buffer_amd import _lib, ops
    new = ops.CylindricalNet(layers, dev, f24a='all')
    assert new.f24_all and new.f24_layers == [l for l, (w, _, _) in enumerate(layers) if w.shape[0] == 32 or (w.shape[0] == 64 and w.shape[1] % 64)]
    if not older:
        for kw in (dict(f24p=True), dict(f24=False), dict(f24a='out64')):
            with pytest.raises(_lib.BufferHipError, match='only 32-output layers may follow'):
                ops.CylindricalNet(layers, dev, **kw)(torch.zeros((1, layers[0][0].shape[1], 140), device=dev))
        return [new, ops.CylindricalNet(layers, dev, f24a='out32')]
    nets = [new, ops.CylindricalNet(layers, dev, f24p=True), ops.CylindricalNet(layers, dev, f24=False)]
    assert nets[1].form == 1 and list(nets[0]._re) == list(nets[1]._re) and not nets[1].f24_layers and not nets[2].f24_layers
    return nets


@pytest.fixture(scope="module")
def released(dev):
    from buffer_amd import ops
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    pe = PatchEmbedder(load_weights("3dmatch"), dev, THREEDMATCH)
    nets = nets_of(pe.layers, dev)
    assert list(nets[0]._re) == [1, 5, 3, 3, 5, 5, 1, 0] and nets[0].f24_layers == RELEASED_NEW
    if ops.F24A_DEFAULT == 'all':
        assert ops.CylindricalNet(pe.layers, dev).f24_all
    return pe.layers, nets


def random_layers(widths, seed=24):
    rng = np.random.default_rng(seed)
    layers = []
    for l in range(8):
        cin, cout = widths[l], widths[l + 1]
        w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)     # keeps the activations' scale
        layers.append((w, (rng.standard_normal(cout) * 0.1).astype(np.float32), l < 7))
    return layers


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
    assert e6 < BOUND and e05 < BOUND and e_all < BOUND
    assert all(o < 2 * BOUND for o in others)
    return ys[0]


@pytest.mark.parametrize("channel", [0, 47])
def test_impulses_at_every_position(released, dev, channel):
    """Patch p holds a single 1.0 at map position p of one input channel: every window of layer 0, row 6, columns 16..19 and the azimuth
    wrap included; channel 47 is the last of layer 0's third k-loop iteration."""
    layers, nets = released
    x = torch.zeros((140, 48, 140))
    x[torch.arange(140), channel, torch.arange(140)] = 1.0
    check(f'impulses in channel {channel}', x.to(dev), layers, nets, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_dense_inputs_and_batch_order(released, dev, n):
    """1, 3 and 513 patches (one more than the 512 workgroups a launch holds at once), signed and non-negative; a permuted batch gives
    the permuted result bit for bit."""
    layers, nets = released
    g = torch.Generator(device='cpu').manual_seed(2600 + n)
    for signed in (True, False):
        x = torch.rand((n, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        y = check(f'n = {n}, {"signed" if signed else "non-negative"}', x, layers, nets, dev)
        perm = torch.randperm(n, generator=g).to(dev)
        assert torch.equal(nets[0](x[perm]), y[perm])


@pytest.mark.parametrize("n", [1, 3, 513])
def test_stack_a(stack_a, dev, n):
    layers, nets = stack_a
    g = torch.Generator(device='cpu').manual_seed(70 + n)
    for signed in (True, False):
        x = torch.rand((n, 48, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'stack A, n = {n}, signed={signed}', x, layers, nets, dev)


@pytest.mark.parametrize("n", [1, 3, 513])
def test_stack_b(stack_b, dev, n):
    layers, nets = stack_b
    g = torch.Generator(device='cpu').manual_seed(90 + n)
    for signed in (True, False):
        x = torch.rand((n, 16, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        check(f'stack B, n = {n}, signed={signed}', x, layers, nets, dev)


def single_tap(layers, layer, tap):
    """Layer `layer` with one tap at (a, b) and the identity over the channels: output o takes input o mod Cin, and where Cin is twice
    Cout half of input Cout + o as well, so both K halves count -- the layer's output is a shifted copy of its input, and a row component
    that enters with the wrong sign, from the wrong window row or into the wrong N-tile shows as a negated, shifted or permuted copy."""
    w, b, relu = layers[layer]
    cout, cin = w.shape[:2]
    w = np.zeros_like(w)
    o = np.arange(cout)
    w[o, o % cin, tap // 3, tap % 3] = 1.0
    if cin == 2 * cout:
        w[o, cout + o, tap // 3, tap % 3] = 0.5
    layers[layer] = (w, b, relu)
    return layers


@pytest.mark.parametrize("layer", [0, 5])
@pytest.mark.parametrize("tap", range(9))
def test_single_tap_filters(dev, input_b, layer, tap):
    """Stack B's layer 0 (16 -> 64) and its first 32-output layer (64 -> 32)"""
    layers = single_tap(random_layers(STACK_B), layer, tap)
    check(f'layer {layer}, tap ({tap // 3}, {tap % 3})', input_b, layers, nets_of(layers, dev), dev)


@pytest.mark.parametrize("layer", [0, 5])
def test_zero_filters_and_a_random_bias(dev, input_b, layer):
    """The layer's output is relu(bias) at every position: a bias that more than one row component carries, or that both K halves of the
    direct round carry, shows as a multiple."""
    layers = random_layers(STACK_B)
    w, b, relu = layers[layer]
    b = np.random.default_rng(5).standard_normal(b.shape).astype(np.float32)
    layers[layer] = (np.zeros_like(w), b, relu)
    check(f'layer {layer}, bias only', input_b, layers, nets_of(layers, dev), dev)


def test_a_width_no_form_takes(dev):
    """A 64 -> 64 layer widened to Cin = 72 (72 % 16 = 8) behind a 64 -> 72 layer: the net built without a form argument does what
    f24p=True does on the same stack.  No kernel of the library runs such widths (output widths are 32, 64 or 128 and every k-loop runs
    four k-steps per iteration), so what both do is refuse: the classes in the filter tiling (an AssertionError of
    ops.winograd_tile_weights on the 72 outputs), and the entry points behind them, called directly on device buffers, with
    'unsupported widths' (BUF_EINVAL) before anything is launched."""
    from buffer_amd import _lib, ops
    widths = [48, 64, 72, 64, 128, 64, 64, 32, 32]
    layers = random_layers(widths)
    assert layers[2][0].shape[:2] == (64, 72)
    x = torch.zeros((2, 48, 140), device=dev)
    for kw in (dict(), dict(f24p=True)):
        with pytest.raises(AssertionError) as e:
            ops.CylindricalNet(layers, dev, **kw)(x)
        assert e.traceback[-1].name == 'winograd_tile_weights'
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=dev)
    ptrs = (C.c_void_p * 8)(*[buf.data_ptr()] * 8)
    ci, co, re_ = (C.c_int * 8)(*widths[:8]), (C.c_int * 8)(*widths[1:]), (C.c_int * 8)(1, 1, 1, 3, 5, 5, 1, 0)
    y = torch.empty((2, 32, 140), device=dev)
    said = []
    assert L.buf_cylindrical_net_wg_all(ops._ptr(x), 2, ptrs, ptrs, ci, co, re_, (C.c_void_p * 8)(), ops._ptr(y), ops._stream()) == -1
    said.append(L.buf_last_error())
    assert L.buf_cylindrical_net_wg_form(ops._ptr(x), 2, ptrs, ptrs, ci, co, re_, 1, ops._ptr(y), ops._stream()) == -1
    said.append(L.buf_last_error())
    assert said[0] == said[1] and b'layer 1 has unsupported widths 64 -> 72' in said[0], said


def test_the_older_forms_in_the_new_kernel_bit_for_bit(released, dev):
    """buf_cylindrical_net_wg_all without a single F(2x4) set of a layer's own runs the layer forms of buf_cylindrical_net_wg_form (pass
    split) in every layer -- the 64-output layers 1, 4 and 5 among them, whose form the two share when the sets are there as well: bit for
    bit that entry point's output (both reach k_cyl_net_w25t: cyl_prepare hands it the same parameters)."""
    from buffer_amd import _lib, ops
    layers, nets = released
    old = nets[1]
    g = torch.Generator(device='cpu').manual_seed(41)
    x = (torch.rand((67, 48, 140), generator=g) * 2 - 1).to(dev)
    y = torch.empty((67, 32, 7, 20), dtype=torch.float32, device=dev)
    none = (C.c_void_p * 8)()
    ops.check(_lib.lib().buf_cylindrical_net_wg_all(ops._ptr(x), 67, old._wp, old._bp, old._ci, old._co, old._re, none, ops._ptr(y), ops._stream()),
              "buf_cylindrical_net_wg_all")
    assert torch.equal(y.view(torch.int32), old(x).view(torch.int32))


def test_masked_rerun_takes_the_same_kernel(released, dev):
    """Through ops.CylindricalNetSplit the fp32 re-run of the flagged patches (an overflowing patch, a NaN) is k_cyl_net_w25t_rerun: the
    plain call's result, bit for bit."""
    from buffer_amd import ops
    layers, nets = released
    split = ops.CylindricalNetSplit(layers, dev, f24a='all')
    assert split.safe and split.f24_all and split.f24_layers == RELEASED_NEW and list(split._re_safe) == [1, 5, 3, 3, 5, 5, 1, 0]
    g = torch.Generator(device='cpu').manual_seed(78)
    bad = torch.rand((23, 48, 140), generator=g).to(dev)
    bad[2] *= 1e6
    bad[22, 47, 139] = float('nan')
    y, y32 = split(bad), nets[0](bad)
    rows = sorted(np.nonzero(split.last_flags.cpu().numpy())[0].tolist())
    assert rows == [2, 22]
    rr = torch.tensor(rows, device=dev)
    assert torch.equal(y[rr].view(torch.int32), y32[rr].view(torch.int32))            # bitwise, NaN patterns included
