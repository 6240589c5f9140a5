"""Pin tests/vn_ref.py (the float64 references of tests/test_vn_kernels_gpu.py) against oracle/torch_ref.py evaluated in float64: the
two are written independently (numpy from the C ABI's contract with the folded batch-norm, torch from the reference's layers), so
agreement at float64 level says both state the same operation.  Small random inputs with shadows on the released 3DMatch weights,
then block 0 and the first resnet block of the committed fixture.  CPU only."""
import os

import numpy as np
import pytest
import torch

import vn_ref
from oracle import torch_ref as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# |vn_ref - torch_ref(float64)| / max|torch_ref|, measured: at most 5.1e-16 over the random inputs (a few hundred rows) and 2.6e-15 on
# the fixture (block 0: 5.4e-16; first resnet block, 2750 x 30 values through three layers: 2.51e-15).  The folded batch-norm and
# numpy's / torch's summation orders are the only differences.  Each limit is within 2x of its measured value.
BOUND_RANDOM = 1e-15
BOUND_FIXTURE = 5e-15


@pytest.fixture(scope="module")
def Wn():
    from buffer_amd.weights import load_weights
    return load_weights("3dmatch")


@pytest.fixture(scope="module")
def W64(Wn):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in Wn.items() if k.startswith(('Ref.', 'Keypt.'))}


def _err(got, want, what, bound=BOUND_RANDOM):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape and got.dtype == np.float64, what
    e = np.abs(got - want).max() / np.abs(want).max()
    print(f'{what}: vn_ref vs torch_ref in float64, max error / scale = {e:.2e}')
    assert e <= bound, (what, e)


def _scene(seed, nq, ns, k, cin, same=False):
    """fp32 inputs of the kind the kernels get; ~20 % shadows (index ns: the only shadow value torch_ref's padded row can express),
    one all-shadow row, one row without, a shadow in slot 0 and in slot K - 1"""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(ns, 3)).astype(np.float32)
    q = s.copy() if same else (s[rng.integers(0, ns, nq)] + rng.normal(scale=0.05, size=(nq, 3))).astype(np.float32)
    nq = len(q)
    feats = rng.normal(size=(ns, 3 * cin)).astype(np.float32)
    idx = rng.integers(0, ns, (nq, k))
    idx[rng.random((nq, k)) < 0.2] = ns
    idx[0], idx[1], idx[2, 0], idx[3, k - 1] = ns, rng.integers(0, ns, k), ns, ns
    return q, s, feats, idx


def _t(a):
    return torch.from_numpy(np.asarray(a)).double() if np.asarray(a).dtype.kind == 'f' else torch.from_numpy(np.asarray(a)).long()


def _resnet(Wn, p, feats, q, s, idx, scale, strided):
    """VNNResnetBlock out of the vn_ref entry points, in the order buffer_amd/point_learner.py calls the kernels"""
    x = vn_ref.gather_block(q, s, feats, idx, *vn_ref.layer(Wn, p + '.conv'), 0.2, 1, scale)
    sc = vn_ref.gather_max(feats, idx) if strided else np.asarray(feats, np.float64)
    sc = vn_ref.pointwise(None, None, sc, *vn_ref.layer(Wn, p + '.unary_shortcut'), 0.2, None)
    return vn_ref.pointwise(None, None, x, *vn_ref.layer(Wn, p + '.unary'), 0.2, sc)


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_gather_blocks_random(Wn, W64, scale):
    q, s, f, idx = _scene(1, 70, 50, 7, 1)
    got = vn_ref.gather_block(q, s, f, idx, *vn_ref.layer(Wn, 'Ref.encoder_blocks.0.conv'), 0.2, 6, scale)
    _err(got, T.vnn_block(_t(f), _t(q), _t(s), _t(idx), W64, 'Ref.encoder_blocks.0', '6', scale), 'vnn_block mode 6')
    assert np.array_equal(got[0], np.zeros(30))                               # the all-shadow row
    q, s, f, idx = _scene(2, 60, 45, 6, 10)
    got = vn_ref.gather_block(q, s, f, idx, *vn_ref.layer(Wn, 'Ref.encoder_blocks.1.conv'), 0.2, 1, scale)
    _err(got, T.vnn_block(_t(f), _t(q), _t(s), _t(idx), W64, 'Ref.encoder_blocks.1', '1', scale), 'vnn_block mode 1')
    assert np.array_equal(got[0], np.zeros(15))


def test_shadow_values_above_ns_are_shadows(Wn):
    """the contract is idx >= ns (torch_ref can only express idx == ns)"""
    q, s, f, idx = _scene(3, 40, 30, 5, 1)
    idx2 = np.where((idx == 30) & (np.arange(40)[:, None] % 2 == 0), 35, idx)
    L = vn_ref.layer(Wn, 'Ref.encoder_blocks.0.conv')
    assert np.array_equal(vn_ref.gather_block(q, s, f, idx, *L, 0.2, 6, 1.0), vn_ref.gather_block(q, s, f, idx2, *L, 0.2, 6, 1.0))
    f30 = np.random.default_rng(0).normal(size=(30, 30)).astype(np.float32)
    assert np.array_equal(vn_ref.gather_max(f30, idx), vn_ref.gather_max(f30, idx2))
    a = np.random.default_rng(2).normal(size=(30, 60)).astype(np.float32)
    W2 = vn_ref.layer(Wn, 'Ref.decoder_blocks.1.mlp')
    sk = np.random.default_rng(3).normal(size=(40, 120)).astype(np.float32)
    assert np.array_equal(vn_ref.pointwise(a, idx[:, 0], sk, *W2, 0.2, None), vn_ref.pointwise(a, idx2[:, 0], sk, *W2, 0.2, None))


@pytest.mark.parametrize("strided", [True, False])
def test_resnet_block_random(Wn, W64, strided):
    p = 'Ref.encoder_blocks.1' if strided else 'Ref.encoder_blocks.2'
    q, s, f, idx = _scene(4 + strided, 50, 40, 6, 10, same=not strided)
    got = _resnet(Wn, p, f, q, s, idx, 1.0, strided)
    _err(got, T.vnn_resnet_block(_t(f), _t(q), _t(s), _t(idx), W64, p, 1.0, strided), f'vnn_resnet_block strided={strided}')


def test_pools_and_vn_block_random(Wn, W64):
    q, s, f, idx = _scene(6, 50, 40, 6, 10)
    assert np.array_equal(vn_ref.gather_max(f, idx), T.max_pool(_t(f), _t(idx)).numpy())
    neg = -np.abs(f) - 1
    assert np.array_equal(vn_ref.gather_max(neg, idx), T.max_pool(_t(neg), _t(idx)).numpy())
    # closest_pool + skip concat + VNBlock (decoder block 3: 20 upsampled + 10 skip channels)
    rng = np.random.default_rng(7)
    y = rng.normal(size=(40, 60)).astype(np.float32)
    skip = rng.normal(size=(50, 30)).astype(np.float32)
    want = T.vn_block(torch.cat([T.closest_pool(_t(y), _t(idx)), _t(skip)], 1), W64, 'Ref.decoder_blocks.3')
    got = vn_ref.pointwise(y, idx[:, 0], skip, *vn_ref.layer(Wn, 'Ref.decoder_blocks.3.mlp'), 0.2, None)
    _err(got, want, 'closest_pool + vn_block')
    assert (idx[:, 0] == 40).any()                                            # (a shadow in column 0 is among the rows)
    # a layer of one output channel: no batch-norm
    x = rng.normal(size=(50, 15)).astype(np.float32)
    L = vn_ref.layer(Wn, 'Ref.fc_layer.1')
    assert L[2] is None and L[3] is None
    _err(vn_ref.pointwise(None, None, x, *L, 0.2, None), T._from_vn(T.vn_linear_leaky(T._to_vn(_t(x)), W64, 'Ref.fc_layer.1')), 'fc_layer.1')


@pytest.mark.parametrize("p", ['Ref.inv_layer', 'Keypt.invar_layer'])
def test_score_head_contraction_random(Wn, W64, p):
    """VNStdFeature: vn1 -> vn2 (slope 0) -> vn_lin (plain VN linear) -> x . z"""
    x = np.random.default_rng(8).normal(size=(45, 30)).astype(np.float32)
    x_vn = T._to_vn(_t(x))
    z = T.vn_linear_leaky(T.vn_linear_leaky(x_vn, W64, p + '.0.vn1', slope=0.0), W64, p + '.0.vn2', slope=0.0)
    z = torch.einsum('oc,bc...->bo...', W64[p + '.0.vn_lin.weight'], z)
    want = torch.einsum('bijm,bkjm->bikm', x_vn, z).reshape(1, -1, 45)[0].transpose(0, 1)
    zr = vn_ref.pointwise(None, None, x, *vn_ref.layer(Wn, p + '.0.vn1'), 0.0, None)
    zr = vn_ref.pointwise(None, None, zr, *vn_ref.layer(Wn, p + '.0.vn2'), 0.0, None)
    zr = vn_ref.pointwise(None, None, zr, np.asarray(Wn[p + '.0.vn_lin.weight'], np.float64), None, None, None, 0.0, None)
    _err(zr, T._from_vn(z), 'vn1 -> vn2 -> vn_lin')
    _err(vn_ref.vn_std(x, zr), want, 'x . z')


def test_fixture_block0_and_first_resnet_block(Wn, W64):
    g = np.load(os.path.join(GOLD, "pyramid_tiny.npz"), allow_pickle=False)
    f = np.load(os.path.join(GOLD, "point_learner_tiny.npz"), allow_pickle=False)
    p0, p1, n0, po0 = g['points_0'], g['points_1'], g['neighbors_0'], g['pools_0']
    with torch.no_grad():
        w0 = T.vnn_block(_t(f['features']), _t(p0), _t(p0), _t(n0), W64, 'Ref.encoder_blocks.0', '6', 1.0)
    x0 = vn_ref.gather_block(p0, p0, f['features'], n0, *vn_ref.layer(Wn, 'Ref.encoder_blocks.0.conv'), 0.2, 6, 1.0)
    _err(x0, w0, 'fixture block 0', BOUND_FIXTURE)
    # each side continues from the fixture's own fp32 block 0, so the second comparison does not inherit the first one's difference
    with torch.no_grad():
        w1 = T.vnn_resnet_block(_t(f['block0']), _t(p1), _t(p0), _t(po0), W64, 'Ref.encoder_blocks.1', 1.0, True)
    _err(_resnet(Wn, 'Ref.encoder_blocks.1', f['block0'], p1, p0, po0, 1.0, True), w1, 'fixture resnet block 1', BOUND_FIXTURE)
