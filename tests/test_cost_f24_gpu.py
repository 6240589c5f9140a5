"""The forms of csrc/costnet_w24.hip (F(2x4) tiles in layers 2 and 4, the Winograd F(2x2) form in layer 6) on the GPU: the released
weights against library convolutions, fixture F5 and the network in float64; synthetic weights that make a wrong window row, tap, tile
origin or a leaking padded column an error of order one; and the bit-for-bit properties of the entry points.  m = 1, 3 and 70 matches.

The bound against float64 is 1e-4 on ind in [0, 20), the one tests/test_model_gpu.py holds the cost-net kernels to.  The synthetic nets
are brought into the conditioning that bound was set for: their last layer is rescaled (from the float64 evaluation, before any kernel
runs) so that the 20 logits have unit spread, as a trained net's have -- ind then moves by at most 19 x the largest logit error, and an
O(1) error in one activation moves it by 1e-2 or more."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as T  # noqa: E402  (test-side torch restatement)
from test_cost_f24_cpu import random_layers

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PARTS = ('all', 'l2', 'l4', 'l6')
BOUND = 1e-4


@pytest.fixture(scope='module')
def W():
    from buffer_amd.weights import load_weights
    return load_weights('3dmatch')


@pytest.fixture(scope='module')
def maps(dev):
    """70 random normalised map pairs, seed 1 (as in test_fused_cost_volume_vs_library_convs)"""
    g = torch.Generator(device='cpu').manual_seed(1)
    a = F.normalize(torch.rand((70, 32, 5, 20), generator=g), dim=1).to(dev)
    b = F.normalize(torch.rand((70, 32, 5, 20), generator=g), dim=1).to(dev)
    return a, b


def logits64(layers, a, b):
    """the network in float64 (folded layers: convolution + ReLU, the last without) -> [m, 20] logits"""
    cols = torch.stack([torch.roll(torch.arange(20), i) for i in range(20)]).to(a.device)
    a, b = a.double(), b.double()
    s = a[:, :, :, cols.reshape(-1)].reshape(a.shape[0], 32, 5, 20, 20).permute(0, 1, 3, 2, 4)
    x = s - b.unsqueeze(2)
    for i, (w, bias) in enumerate(layers):
        x = F.conv3d(x, torch.from_numpy(np.asarray(w, np.float64)).to(a.device), torch.from_numpy(np.asarray(bias, np.float64)).to(a.device))
        x = F.relu(x) if i < 9 else x
    return x.reshape(x.shape[0], -1)


def ind64(layers, a, b):
    p = torch.softmax(logits64(layers, a, b), dim=-1)
    return (p * torch.arange(20, device=a.device, dtype=torch.float64)[None]).sum(-1)


def calibrated(layers, a, b):
    """the layers with the last one rescaled so that the logits of (a, b) have unit standard deviation in float64"""
    s = float(logits64(layers, a, b).std())
    assert np.isfinite(s) and s > 0
    w9, b9 = layers[9]
    return layers[:9] + [((w9 / s).astype(np.float32), (b9 / s).astype(np.float32))]


def check_forms(layers, a, b, dev, forms, what):
    """every form of `forms` and 'off' against float64; prints the figures, then asserts the bound for the new forms"""
    from buffer_amd import ops
    ref = ind64(layers, a, b)
    spread = float(ref.std()) if ref.numel() > 1 else 0.0
    errs = {f: float((ops.CostVolumeNet(layers, dev, f24=f)(a, b).double() - ref).abs().max()) for f in tuple(forms) + ('off',)}
    print(f'{what}, m = {a.shape[0]} (ind spread {spread:.2f}): max |ind - ind64| ' + ', '.join(f'{f} {e:.2e}' for f, e in errs.items()))
    for f in forms:
        assert errs[f] < BOUND, (what, f, errs)
    return errs


def test_released_weights(W, dev, maps):
    """Every part alone and all three: against library convolutions and fixture F5 at the fp32 kernel's tolerance, against float64 below
    1e-4 (printed beside the F(2x2) kernel's figure on the same input)."""
    from buffer_amd import registration
    f = np.load(os.path.join(GOLD, 'match_tiny.npz'), allow_pickle=False)
    se = torch.from_numpy(f['src_equi'])[f['s_mids']][:, :, 1:6].contiguous().to(dev)
    te = torch.from_numpy(f['tgt_equi'])[f['t_mids']][:, :, 1:6].contiguous().to(dev)
    a, b = maps
    Wd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in W.items()}
    W64 = {k: v.double() for k, v in Wd.items() if k.startswith('Inlier')}
    want_g, want_r = T.cost_volume(se, te, Wd).cpu().numpy(), T.cost_volume(a, b, Wd).cpu().numpy()
    ref_g, ref_r = T.cost_volume(se.double(), te.double(), W64), T.cost_volume(a.double(), b.double(), W64)
    off = registration.CostVolume(W, dev, f24='off')
    e_off = max(float((off(se, te).double() - ref_g).abs().max()), float((off(a, b).double() - ref_r).abs().max()))
    for part in PARTS:
        cv = registration.CostVolume(W, dev, f24=part)
        got_g, got_r = cv(se, te), cv(a, b)
        e = max(float((got_g.double() - ref_g).abs().max()), float((got_r.double() - ref_r).abs().max()))
        print(f'released weights, {part}: max |ind - ind64| = {e:.2e} (F(2x2) kernel on the same inputs: {e_off:.2e})')
        np.testing.assert_allclose(got_g.cpu().numpy(), want_g, rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(got_g.cpu().numpy(), f['ind'], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(got_r.cpu().numpy(), want_r, rtol=1e-4, atol=2e-4)
        assert e < BOUND
    with pytest.raises(ValueError):
        registration.CostVolume(W, dev, f24='some')


@pytest.mark.parametrize('m', [1, 3, 70])
def test_random_layers(dev, maps, m):
    a, b = maps[0][:m].contiguous(), maps[1][:m].contiguous()
    layers = calibrated(random_layers(11), *maps)
    check_forms(layers, a, b, dev, PARTS, 'random layers')


@pytest.mark.parametrize('layer', [2, 4, 6])
def test_single_tap_filters(dev, maps, layer):
    """The layer's filters have one non-zero tap (dn, dl): its output is a channel mix of the input shifted by the tap.  A wrong window row,
    tap or tile origin in the new form reads another shift: an error of order one.  The part alone at every tap, all three parts at two."""
    a, b = maps[0][:3].contiguous(), maps[1][:3].contiguous()
    base = random_layers(12)
    rng = np.random.default_rng(layer)
    cout, cin = base[layer][0].shape[:2]
    mix = (rng.standard_normal((cout, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
    for tap in range(9):
        w = np.zeros_like(base[layer][0])
        w[:, :, tap // 3, 0, tap % 3] = mix
        layers = calibrated(base[:layer] + [(w, base[layer][1])] + base[layer + 1:], a, b)
        check_forms(layers, a, b, dev, (f'l{layer}', 'all') if tap in (0, 8) else (f'l{layer}',), f'layer {layer}, single tap {tap // 3, tap % 3}')


@pytest.mark.parametrize('layer', [2, 4, 6])
def test_zero_filters_with_a_random_bias(dev, maps, layer):
    """The layer's output is its bias at every position: the bias must reach every kept output once (column component 1 of the F(2x4)
    form, component (1, 1) of the F(2x2) form)."""
    a, b = maps[0][:3].contiguous(), maps[1][:3].contiguous()
    base = random_layers(13)
    rng = np.random.default_rng(layer)
    bias = rng.standard_normal(base[layer][0].shape[0]).astype(np.float32)
    # (identical outputs for every match would give the logits no spread over the matches: the spread over the 20 logits is what counts)
    layers = calibrated(base[:layer] + [(np.zeros_like(base[layer][0]), bias)] + base[layer + 1:], a, b)
    check_forms(layers, a, b, dev, (f'l{layer}', 'all'), f'layer {layer}, zero filters')


@pytest.mark.parametrize('layer', [2, 4])
def test_large_positive_inputs(dev, maps, layer):
    """A bias of +8 in the layer before makes every word of the layer's input large and positive, the words the last tile column reads past
    its row included: one that leaked into a kept output column would move it by the order of the input.  m = 3 and m = 1."""
    base = random_layers(14)
    wb, bb = base[layer - 1]
    for m in (3, 1):
        a, b = maps[0][:m].contiguous(), maps[1][:m].contiguous()
        layers = calibrated(base[:layer - 1] + [(wb, (bb + 8).astype(np.float32))] + base[layer:], maps[0][:3], maps[1][:3])
        check_forms(layers, a, b, dev, (f'l{layer}', 'all'), f'layer {layer}, inputs + 8')


def test_bit_for_bit(W, dev, maps):
    """The gather form equals the dense form; a permuted batch gives the permuted result; the masked re-run equals the plain call on the
    flagged matches and leaves the others untouched; 'off' is the entry point without sets (every layer in its first form) and
    equals the entry point of three sets with all three null, which guards the slots the host side fills for each; no matches: an empty tensor."""
    from buffer_amd import _lib, registration
    from buffer_amd.ops import _ptr, _stream
    a, b = maps
    cv = registration.CostVolume(W, dev, f24='all')
    g = torch.Generator(device='cpu').manual_seed(4)
    equi = F.normalize(torch.rand((120, 32, 7, 20), generator=g), dim=1).to(dev)
    s_rows = torch.randint(0, 120, (70,), generator=g).to(dev)
    t_rows = torch.randint(0, 120, (70,), generator=g).to(dev)
    dense = cv(equi[s_rows][:, :, 1:6].contiguous(), equi[t_rows][:, :, 1:6].contiguous())
    assert torch.equal(cv.gathered(equi, s_rows, t_rows), dense)
    assert cv.gathered(equi, s_rows[:0], t_rows[:0]).shape == (0,) and cv(a[:0], b[:0]).shape == (0,)
    full = cv(a, b)
    perm = torch.randperm(70, generator=g).to(dev)
    assert torch.equal(cv(a[perm].contiguous(), b[perm].contiguous()), full[perm])
    assert torch.equal(cv(a[:1].contiguous(), b[:1].contiguous()), full[:1]) and torch.equal(cv(a[:3].contiguous(), b[:3].contiguous()), full[:3])
    # 'off' and the kernel without sets
    off = registration.CostVolume(W, dev, f24='off')
    want_off = off(a, b)
    net = off.fused
    out = torch.empty((70,), dtype=torch.float32, device=dev)
    L = _lib.lib()
    assert L.buf_cost_volume_net(_ptr(a), _ptr(b), 70, net._wp, net._bp, _ptr(out), _stream()) == 0
    assert torch.equal(out, want_off)
    out2 = torch.empty((70,), dtype=torch.float32, device=dev)
    assert L.buf_cost_volume_net_w24(_ptr(a), _ptr(b), 70, net._wp, net._bp, (C.c_void_p * 3)(), _ptr(out2), _stream()) == 0
    assert torch.equal(out2, want_off)
    assert not torch.equal(full, want_off)                 # (the new forms round differently: the switch does something)
    # the masked re-run: matches beyond the f16 range go through the masked twin by buf_cost_volume_net_split_safe_w24
    for part in ('all', 'l4'):
        cv32 = registration.CostVolume(W, dev, f24=part)
        cvs = registration.CostVolume(W, dev, arith='split', f24=part)
        assert cvs.fused.safe
        clean = cvs(a, b)
        assert cvs.fused.range_fallbacks() == 0
        a2 = a.clone()
        a2[5] *= 1e6
        a2[69, 1, 2, 3] = float('nan')
        want, got = cv32(a2, b), cvs(a2, b)
        fl = sorted(np.nonzero(cvs.fused.last_flags.cpu().numpy())[0].tolist())
        assert fl == [5, 69]
        keep = torch.tensor([i for i in range(70) if i not in fl], device=dev)
        ff = torch.tensor(fl, device=dev)
        assert torch.equal(got[keep], clean[keep]) and torch.equal(got[ff].view(torch.int32), want[ff].view(torch.int32))
        cvs.fused.check_range()
