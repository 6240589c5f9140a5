"""The descriptor CNN's bottom map row (output row 6) in the direct two-row form (csrc/convnet_wg.hip, wg_round_direct): columns 0..15
are one full M-tile of 16 positions, columns 16..19 stay Winograd tiles.  Inputs that single out that row and its seams, against the
float64 stack and the direct-form test kernel, under the bound of test_winograd_and_direct_forms_against_float64 (1e-5 of the output
scale: fp32 accumulation over K <= 9 x 128 products per output leaves ~1e-7 x sqrt(K) of the scale per layer, eight layers)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BOUND = 1e-5


@pytest.fixture(scope="module")
def W():
    from buffer_amd.weights import load_weights
    return load_weights("3dmatch")


def stack64(x, layers, dev):
    h = x.double().reshape(-1, layers[0][0].shape[1], 7, 20)
    for w, b, relu in layers:                                                # circular azimuth, zero elevation, float64
        h = torch.cat([h[..., -1:], h, h[..., :1]], -1)
        h = torch.nn.functional.pad(h, (0, 0, 1, 1))
        h = torch.nn.functional.conv2d(h, torch.from_numpy(np.ascontiguousarray(w)).double().to(dev),
                                       torch.from_numpy(np.ascontiguousarray(b)).double().to(dev))
        h = torch.relu(h) if relu else h
    return h


def errors(y, h):
    """(whole map, row 6, rows 0..5): max |y - h| over the output scale of the whole map"""
    scale = h.abs().max().item()
    d = (y.double() - h).abs()
    return d.max().item() / scale, d[:, :, 6].max().item() / scale, d[:, :, :6].max().item() / scale, scale


def masked_inputs(g, n=24):
    """name -> x [n, 48, 7, 20] (the kernel's [n, 16, 420] input seen as the 48-channel map)"""
    base = torch.rand((n, 48, 7, 20), generator=g) * 2 - 1
    def only(rows=slice(None), cols=slice(None)):
        x = torch.zeros_like(base)
        x[:, :, rows, cols] = base[:, :, rows, cols]
        return x
    return {
        'rows 5 and 6 only': only(rows=[5, 6]),
        'row 6 only': only(rows=[6]),
        'row 5 only': only(rows=[5]),
        'column 19 only': only(cols=[19]),                     # wraps into p - 1 at p = 0 of the direct M-tile
        'column 0 only': only(cols=[0]),                       # wraps out of it into the Winograd tile of column 19
        'columns 15 and 16 only': only(cols=[15, 16]),         # the seam between the direct M-tile and the Winograd tiles of 16..19
        'dense signed': base,
        'dense non-negative': base.abs(),
    }


def test_bottom_row_and_its_seams_against_float64_and_the_direct_kernel(W, dev):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from util import DirectCylindricalNet
    pe = PatchEmbedder(W, dev, THREEDMATCH)
    assert pe.fused.entry == "buf_cylindrical_net_wg"
    direct = DirectCylindricalNet(pe.layers, dev)
    g = torch.Generator(device='cpu').manual_seed(11)
    failed = []
    for name, x4 in masked_inputs(g).items():
        x = x4.reshape(-1, 16, 420).to(dev)
        h = stack64(x, pe.layers, dev)
        y, yd = pe.fused(x), direct(x)
        e_all, e6, e05, scale = errors(y, h)
        d_all, d6, _, _ = errors(yd, h)
        x_all = (y - yd).abs().max().item() / scale
        x6 = (y[:, :, 6] - yd[:, :, 6]).abs().max().item() / scale
        print(f'{name:24s} scale {scale:9.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e} | direct kernel vs float64: '
              f'all {d_all:.2e} row 6 {d6:.2e} | vs direct kernel: all {x_all:.2e} row 6 {x6:.2e}')
        if not (e_all < BOUND and e6 < BOUND and x_all < BOUND and x6 < BOUND):
            failed.append(name)
    assert not failed, failed


@pytest.mark.parametrize("n", [1, 3, 700])
def test_patch_counts_and_batch_permutation(W, dev, n):
    """1, 3 and a count that is not a multiple of 512 (nor of the 256 CUs x 2 workgroups): every patch against float64, and bit-identical
    under a permutation of the batch."""
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    pe = PatchEmbedder(W, dev, THREEDMATCH)
    g = torch.Generator(device='cpu').manual_seed(100 + n)
    x = torch.rand((n, 16, 420), generator=g).to(dev)
    y = pe.fused(x)
    e_all, e6, e05, _ = errors(y, stack64(x, pe.layers, dev))
    print(f'n = {n}: vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e}')
    assert e_all < BOUND and e6 < BOUND
    perm = torch.randperm(n, generator=g).to(dev)
    assert torch.equal(pe.fused(x[perm]), y[perm])


def test_second_stack_moves_the_k_ranges_of_every_layer_form(dev):
    """64 inputs; 64, 64, 128, 128, 64, 64, 32, 32 outputs with random filters through ops.CylindricalNet: other K ranges (and k-loop trip
    counts) in the 64-, 128- and 32-channel layer forms than the released stack has."""
    from buffer_amd import _lib, ops
    import ctypes as C
    widths = [64, 64, 64, 128, 128, 64, 64, 32, 32]
    ci, co = (C.c_int * 8)(*widths[:-1]), (C.c_int * 8)(*widths[1:])
    assert _lib.lib().buf_cylindrical_net_wg_supports(ci, co) == 0
    rng = np.random.default_rng(3)
    layers = []
    for l in range(8):
        cin, cout = widths[l], widths[l + 1]
        w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)     # keeps the activations' scale
        b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        layers.append((w, b, l < 7))
    net = ops.CylindricalNet(layers, dev)
    g = torch.Generator(device='cpu').manual_seed(9)
    for signed in (False, True):
        x = torch.rand((37, 64, 140), generator=g)
        x = (x * 2 - 1 if signed else x).to(dev)
        y = net(x)
        e_all, e6, e05, scale = errors(y, stack64(x, layers, dev))
        print(f'signed={signed}: scale {scale:.3e} | vs float64: all {e_all:.2e} row 6 {e6:.2e} rows 0..5 {e05:.2e}')
        assert e_all < BOUND and e6 < BOUND
