"""The forms of csrc/costnet_w24b.hip (layer 1 on F(2x4) tiles, one k' plane resident at a time; layer 3 as F(2x4) rows with an F(2x2)
tail) on the GPU: the released weights against library convolutions, fixture F5 and the network in float64; synthetic weights and inputs
that make a wrong plane, tap, tile origin, seam or a bias added per plane an error of order one; and the bit-for-bit properties of the
entry points.  m = 1, 3 and 70 matches.

The bound against float64 is 1e-4 on ind in [0, 20), with the synthetic nets calibrated to logits of unit spread, as in
tests/test_cost_f24_gpu.py (whose helpers these are)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as T  # noqa: E402  (test-side torch restatement)
from test_cost_f24_cpu import random_layers
from test_cost_f24_gpu import BOUND, calibrated, ind64

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PARTS = ('all', 'l1', 'l3')


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


def check_forms(layers, a, b, dev, forms, what):
    """every form of `forms` and 'off' (f24 = 'all' alone) against float64; prints the figures, then asserts the bound for the new forms"""
    from buffer_amd import ops
    ref = ind64(layers, a, b)
    spread = float(ref.std()) if ref.numel() > 1 else 0.0
    errs = {f: float((ops.CostVolumeNet(layers, dev, f24b=f)(a, b).double() - ref).abs().max()) for f in tuple(forms) + ('off',)}
    print(f'{what}, m = {a.shape[0]} (ind spread {spread:.2f}): max |ind - ind64| ' + ', '.join(f'{f} {e:.2e}' for f, e in errs.items()))
    for f in forms:
        assert errs[f] < BOUND, (what, f, errs)
    return errs


def test_released_weights(W, dev, maps):
    """Every part alone and both: against library convolutions and fixture F5 at the fp32 kernel's tolerance, against float64 below 1e-4
    (printed beside the figure of f24b = 'off' on the same input)."""
    from buffer_amd import registration
    f = np.load(os.path.join(GOLD, 'match_tiny.npz'), allow_pickle=False)
    se = torch.from_numpy(f['src_equi'])[f['s_mids']][:, :, 1:6].contiguous().to(dev)
    te = torch.from_numpy(f['tgt_equi'])[f['t_mids']][:, :, 1:6].contiguous().to(dev)
    a, b = maps
    Wd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in W.items()}
    W64 = {k: v.double() for k, v in Wd.items() if k.startswith('Inlier')}
    want_g, want_r = T.cost_volume(se, te, Wd).cpu().numpy(), T.cost_volume(a, b, Wd).cpu().numpy()
    ref_g, ref_r = T.cost_volume(se.double(), te.double(), W64), T.cost_volume(a.double(), b.double(), W64)
    off = registration.CostVolume(W, dev, f24b='off')
    e_off = max(float((off(se, te).double() - ref_g).abs().max()), float((off(a, b).double() - ref_r).abs().max()))
    for part in PARTS:
        cv = registration.CostVolume(W, dev, f24b=part)
        got_g, got_r = cv(se, te), cv(a, b)
        eg, er = float((got_g.double() - ref_g).abs().max()), float((got_r.double() - ref_r).abs().max())
        print(f'released weights, {part}: max |ind - ind64| = {eg:.2e} (golden matches), {er:.2e} (random maps); with f24b off on both: {e_off:.2e}')
        np.testing.assert_allclose(got_g.cpu().numpy(), want_g, rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(got_g.cpu().numpy(), f['ind'], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(got_r.cpu().numpy(), want_r, rtol=1e-4, atol=2e-4)
        assert max(eg, er) < BOUND
    with pytest.raises(ValueError):
        registration.CostVolume(W, dev, f24b='some')


@pytest.mark.parametrize('m', [1, 3, 70])
def test_random_layers(dev, maps, m):
    a, b = maps[0][:m].contiguous(), maps[1][:m].contiguous()
    layers = calibrated(random_layers(21), *maps)
    check_forms(layers, a, b, dev, PARTS, 'random layers')


@pytest.mark.parametrize('dk', [0, 1, 2])
def test_layer1_single_tap_filters(dev, maps, dk):
    """Layer 1's filters have one non-zero tap (dk, dn, dl): its output is a channel mix of ONE k' plane shifted by (dn, dl).  A plane or tap
    mix-up, a wrong tile origin or a slip at the seam of the two M-tiles (output rows 7 | 8) reads another shift: an error of order one."""
    a, b = maps[0][:3].contiguous(), maps[1][:3].contiguous()
    base = random_layers(22)
    rng = np.random.default_rng(100 + dk)
    mix = (rng.standard_normal((64, 32)) * np.sqrt(2.0 / 32)).astype(np.float32)
    for tap in range(9):
        w = np.zeros_like(base[1][0])                                   # [o][c][dn][dk][dl]
        w[:, :, tap // 3, dk, tap % 3] = mix
        layers = calibrated(base[:1] + [(w, base[1][1])] + base[2:], a, b)
        check_forms(layers, a, b, dev, ('l1', 'all') if tap in (0, 8) else ('l1',), f'layer 1, single tap dk {dk}, (dn, dl) {tap // 3, tap % 3}')


def test_layer1_single_input_channel(dev, maps):
    """Layer 1 reads one of its 96 collapsed input channels (dk, c) only: the first and last channel of every k' plane."""
    a, b = maps[0][:3].contiguous(), maps[1][:3].contiguous()
    base = random_layers(23)
    rng = np.random.default_rng(5)
    for ch in (0, 31, 32, 63, 64, 95):
        w = np.zeros_like(base[1][0])
        w[:, ch % 32, :, ch // 32, :] = (rng.standard_normal((64, 3, 3)) * np.sqrt(2.0 / 9)).astype(np.float32)
        layers = calibrated(base[:1] + [(w, base[1][1])] + base[2:], a, b)
        check_forms(layers, a, b, dev, ('l1', 'all') if ch in (0, 95) else ('l1',), f'layer 1, input channel {ch} only')


@pytest.mark.parametrize('layer', [1, 3])
def test_zero_filters_with_a_random_bias(dev, maps, layer):
    """The layer's output is its bias at every position: the bias must reach every output once -- in layer 1 once, not once per plane."""
    a, b = maps[0][:3].contiguous(), maps[1][:3].contiguous()
    base = random_layers(24)
    rng = np.random.default_rng(layer)
    bias = rng.standard_normal(base[layer][0].shape[0]).astype(np.float32)
    layers = calibrated(base[:layer] + [(np.zeros_like(base[layer][0]), bias)] + base[layer + 1:], a, b)
    check_forms(layers, a, b, dev, (f'l{layer}', 'all'), f'layer {layer}, zero filters')


def test_layer3_single_tap_filters(dev, maps):
    a, b = maps[0][:3].contiguous(), maps[1][:3].contiguous()
    base = random_layers(25)
    rng = np.random.default_rng(3)
    mix = (rng.standard_normal((128, 64)) * np.sqrt(2.0 / 64)).astype(np.float32)
    for tap in range(9):
        w = np.zeros_like(base[3][0])
        w[:, :, tap // 3, 0, tap % 3] = mix
        layers = calibrated(base[:3] + [(w, base[3][1])] + base[4:], a, b)
        check_forms(layers, a, b, dev, ('l3', 'all') if tap in (0, 8) else ('l3',), f'layer 3, single tap {tap // 3, tap % 3}')


@pytest.mark.parametrize('rows', ['10..13', '0..9'])
def test_layer3_input_rows(dev, rows):
    """Layer 3's input is non-zero only in its rows 10..13 (what the F(2x2) tail reads beyond the F(2x4) rows' last window row 11) or only in
    its rows 0..9.  The maps are built for it: layers 0..2 are single taps at offset 0 with positive channel mixes and no bias, the source
    map is positive at the azimuths j of a set J and zero elsewhere, the target map is large where the column l is to be cut and zero
    elsewhere -- cost[n][l] = S[(l - n) mod 20] - T[l] is then positive on the diagonals l - n in J of the columns kept, negative in the
    columns cut and zero elsewhere, and the ReLUs carry that support to layer 3's input (checked in float64 before any kernel runs)."""
    g = torch.Generator(device='cpu').manual_seed(7)
    m = 3
    a = torch.zeros((m, 32, 5, 20))
    b = torch.zeros((m, 32, 5, 20))
    if rows == '10..13':
        J, cut, keep = [0, 19, 18, 17], slice(0, 10), range(10, 14)       # l - n = 0, -1, -2, -3 and l >= 10: n = l .. l + 3 >= 10
    else:
        J, cut, keep = [0, 1, 2, 3], slice(10, 20), range(0, 10)          # l - n = 0 .. 3 and l <= 9: n <= l <= 9
    a[:, :, :, J] = 0.2 + torch.rand((m, 32, 5, len(J)), generator=g)
    b[:, :, :, cut] = 10.0
    a, b = a.to(dev), b.to(dev)
    base = random_layers(26)
    rng = np.random.default_rng(8)
    layers = list(base)
    for l in range(3):
        w = np.zeros_like(base[l][0])
        cout, cin = w.shape[:2]
        w[:, :, 0, 0, 0] = np.abs(rng.standard_normal((cout, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
        layers[l] = (w, np.zeros(cout, np.float32))
    # layer 3's input in float64: [m, 64, 14, 1, 14]
    cols = torch.stack([torch.roll(torch.arange(20), i) for i in range(20)]).to(dev)
    x = a.double()[:, :, :, cols.reshape(-1)].reshape(m, 32, 5, 20, 20).permute(0, 1, 3, 2, 4) - b.double().unsqueeze(2)
    for w, bias in layers[:3]:
        x = F.relu(F.conv3d(x, torch.from_numpy(w.astype(np.float64)).to(dev), torch.from_numpy(bias.astype(np.float64)).to(dev)))
    assert tuple(x.shape[2:]) == (14, 1, 14)
    live = (x.abs().amax(dim=(0, 1, 3, 4)) > 0).cpu().numpy()
    assert sorted(np.nonzero(live)[0].tolist()) == list(keep), live
    layers = calibrated(layers, a, b)
    check_forms(layers, a, b, dev, ('l3', 'all'), f'layer 3, input rows {rows} only')


@pytest.mark.parametrize('layer', [1, 3])
def test_large_positive_inputs(dev, maps, layer):
    """A bias of +8 in the layer before makes every word of the layer's input large and positive.  m = 3 and m = 1."""
    base = random_layers(27)
    wb, bb = base[layer - 1]
    for m in (3, 1):
        a, b = maps[0][:m].contiguous(), maps[1][:m].contiguous()
        layers = calibrated(base[:layer - 1] + [(wb, (bb + 8).astype(np.float32))] + base[layer:], maps[0][:3], maps[1][:3])
        check_forms(layers, a, b, dev, (f'l{layer}', 'all'), f'layer {layer}, inputs + 8')


def test_bit_for_bit(W, dev, maps):
    """The gather form equals the dense form; a permuted batch gives the permuted result; m = 1 and m = 3 are the first rows of m = 70; the
    masked re-run equals the plain call on the flagged matches and leaves the others untouched; f24b = 'off' is f24 = 'all'
    (the entry point of three sets), and the entry point of five sets without the last two returns the same bits; no matches: an empty tensor."""
    from buffer_amd import _lib, registration
    from buffer_amd.ops import _ptr, _stream
    a, b = maps
    g = torch.Generator(device='cpu').manual_seed(4)
    equi = F.normalize(torch.rand((120, 32, 7, 20), generator=g), dim=1).to(dev)
    s_rows = torch.randint(0, 120, (70,), generator=g).to(dev)
    t_rows = torch.randint(0, 120, (70,), generator=g).to(dev)
    perm = torch.randperm(70, generator=g).to(dev)
    old = registration.CostVolume(W, dev, f24='all')
    want_old = old(a, b)
    for part in PARTS:
        cv = registration.CostVolume(W, dev, f24b=part)
        dense = cv(equi[s_rows][:, :, 1:6].contiguous(), equi[t_rows][:, :, 1:6].contiguous())
        assert torch.equal(cv.fused.gathered(equi, s_rows, t_rows), dense)
        assert cv.fused.gathered(equi, s_rows[:0], t_rows[:0]).shape == (0,) and cv(a[:0], b[:0]).shape == (0,)
        full = cv(a, b)
        assert torch.equal(cv(a[perm].contiguous(), b[perm].contiguous()), full[perm])
        assert torch.equal(cv(a[:1].contiguous(), b[:1].contiguous()), full[:1]) and torch.equal(cv(a[:3].contiguous(), b[:3].contiguous()), full[:3])
        assert not torch.equal(full, want_old)             # (the new forms round differently: the switch does something)
    # 'off', and the kernel without the two sets
    off = registration.CostVolume(W, dev, f24b='off')
    assert off.fused.parts_b == () and torch.equal(off(a, b), want_old)
    net = old.fused
    five = (C.c_void_p * 5)(*[t.data_ptr() for t in net.wt24], None, None)
    out = torch.empty((70,), dtype=torch.float32, device=dev)
    assert _lib.lib().buf_cost_volume_net_w24b(_ptr(a), _ptr(b), 70, net._wp, net._bp, five, _ptr(out), _stream()) == 0
    assert torch.equal(out, want_old)
    # the masked re-run: matches beyond the f16 range go through the masked twin by buf_cost_volume_net_split_safe_w24b
    for part in ('all', 'l1'):
        cv32 = registration.CostVolume(W, dev, f24b=part)
        cvs = registration.CostVolume(W, dev, arith='split', f24b=part)
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
