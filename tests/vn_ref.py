"""Float64 numpy restatement of the vector-neuron entry points of csrc/vn.hip, written from their contracts in
include/buffer_hip.h ("A4/A5 Vector-Neuron blocks") and the layer semantics of oracle/torch_ref.py -- not from the kernels.
tests/test_vn_ref_cpu.py pins it against oracle/torch_ref evaluated in float64; tests/test_vn_kernels_gpu.py compares each kernel
with it.

Feature rows are [N, 3C], channel-major / xyz-minor.  Inputs are the fp32 arrays a kernel gets, widened to `dtype` (float64);
nothing inside is rounded.  dtype=np.float32 evaluates the same formulas in fp32 (numpy keeps fp32 arrays in fp32): the yardstick
"what an fp32 run costs" of the GPU tests, never a reference.  Sums over channels, slots and xyz are written as explicit
element-wise loops, so the fp32 evaluation is one fixed summation order on every machine (numpy's reductions are not).
"""
import numpy as np

EPS = 1e-6          # models/vn_layers.py:10
BN_EPS = 1e-5


def _a(x, dtype):
    return None if x is None else np.asarray(x, dtype)


def fold_bn(W, prefix, dtype=np.float64):
    """VN batch-norm of layer `prefix` in the folded form of the C ABI: bn_scale = w / sqrt(var + 1e-5), bn_shift = b - mean * bn_scale;
    (None, None) for a layer of one output channel (the reference skips VN batch-norm there, vn_layers.py:123)."""
    if np.asarray(W[prefix + '.map_to_feat.weight']).shape[0] == 1:
        return None, None
    g, b, m, v = (np.asarray(W[f'{prefix}.batchnorm.bn.{k}'], np.float64) for k in ('weight', 'bias', 'running_mean', 'running_var'))
    sc = g / np.sqrt(v + BN_EPS)
    return sc.astype(dtype), (b - m * sc).astype(dtype)


def layer(W, prefix, dtype=np.float64):
    """(wf, wd, bn_scale, bn_shift) of the VNLinearLeakyReLU `prefix`."""
    return (np.asarray(W[prefix + '.map_to_feat.weight'], dtype), np.asarray(W[prefix + '.map_to_dir.weight'], dtype)) + fold_bn(W, prefix, dtype)


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _linear(w, inp):
    """VN linear: w [cout, cin], inp [..., cin, 3] -> [..., cout, 3], channels summed in ascending order"""
    acc = np.zeros(inp.shape[:-2] + (w.shape[0], 3), inp.dtype)
    for c in range(w.shape[1]):
        acc = acc + w[:, c, None] * inp[..., c, None, :]
    return acc


def _mean_slots(x):
    """mean over axis 1 (the K slots), slots summed in ascending order"""
    acc = np.zeros_like(x[:, 0])
    for k in range(x.shape[1]):
        acc = acc + x[:, k]
    return acc / x.shape[1]


def vn_epilogue(p, d, bsc, bsh, slope):
    """VN batch-norm with folded scale / shift (skipped when bsc is None), then VN leaky ReLU.  p, d [..., cout, 3]; bsc, bsh [cout].
      norm = |p| + 1e-6;  p <- p / norm * (norm * bsc + bsh)
      dot = <p, d>;  out = slope * p + (1 - slope) * (p  if dot >= 0  else  p - dot / (|d|^2 + 1e-6) * d)"""
    if bsc is not None:
        norm = np.sqrt(_dot3(p, p)) + EPS
        p = p / norm[..., None] * (norm * bsc + bsh)[..., None]
    dot = _dot3(p, d)[..., None]
    dsq = _dot3(d, d)[..., None]
    kept = np.where(dot >= 0, p, p - dot / (dsq + EPS) * d)
    return slope * p + (1 - slope) * kept


def gather_block(q, s, feats, idx, wf, wd, bsc, bsh, slope, mode, scale, dtype=np.float64):
    """buf_vn_gather_block / buf_vn_gather_block_pre: q [nq,3], s [ns,3], feats [ns,3cin], idx int[nq,K] -> [nq, 3cout].
    A slot with idx >= ns is a shadow: delta = 0, features = 0.  Input channels of a slot: mode 1 [f (cin), delta]; mode 6 (cin = 1)
    [f, delta, f x delta, mean of delta over ALL K slots].  VN linear -> epilogue -> mean over ALL K slots."""
    q, s, feats, wf, wd, bsc, bsh = (_a(x, dtype) for x in (q, s, feats, wf, wd, bsc, bsh))
    idx = np.asarray(idx)
    nq, k = idx.shape
    ns, scale = s.shape[0], float(scale)
    cin = feats.shape[1] // 3
    real = idx < ns
    j = np.where(real, idx, ns)
    s_pad = np.concatenate([s, np.zeros((1, 3), dtype)])
    f_pad = np.concatenate([feats.reshape(ns, cin, 3), np.zeros((1, cin, 3), dtype)])
    delta = np.where(real[..., None], (s_pad[j] - q[:, None]) / scale, 0).astype(dtype)      # [nq,K,3]
    f = f_pad[j]                                                                              # [nq,K,cin,3]
    if int(mode) == 1:
        inp = np.concatenate([f, delta[:, :, None]], 2)
    elif int(mode) == 6:
        assert cin == 1
        cross = np.cross(f[:, :, 0], delta)
        mean = np.broadcast_to(_mean_slots(delta)[:, None], delta.shape)
        inp = np.stack([f[:, :, 0], delta, cross, mean], 2)
    else:
        raise ValueError(mode)
    return _mean_slots(vn_epilogue(_linear(wf, inp), _linear(wd, inp), bsc, bsh, slope)).reshape(nq, -1)


def pointwise(a, ind_a, b, wf, wd, bsc, bsh, slope, residual, dtype=np.float64):
    """buf_vn_pointwise: VN layer on concat(a[ind_a] (ca channels), b (cb channels)) (+ residual).  ind_a int[n] (None: identity);
    an index >= len(a) reads as zeros; a or b may be None; wd None = plain VN linear (no batch-norm, no activation)."""
    a, b, wf, wd, bsc, bsh, residual = (_a(x, dtype) for x in (a, b, wf, wd, bsc, bsh, residual))
    parts = []
    if a is not None and a.shape[1] > 0:
        na, ca = a.shape[0], a.shape[1] // 3
        ia = np.arange(na if b is None else b.shape[0]) if ind_a is None else np.asarray(ind_a).reshape(-1)
        a_pad = np.concatenate([a.reshape(na, ca, 3), np.zeros((1, ca, 3), dtype)])
        parts.append(a_pad[np.minimum(ia, na)])
    if b is not None and b.shape[1] > 0:
        parts.append(b.reshape(b.shape[0], -1, 3))
    inp = np.concatenate(parts, 1)                                                            # [n, ca + cb, 3]
    p = _linear(wf, inp)
    if wd is not None:
        p = vn_epilogue(p, _linear(wd, inp), bsc, bsh, slope)
    out = p.reshape(inp.shape[0], -1)
    return out if residual is None else out + residual


def gather_max(feats, idx, dtype=np.float64):
    """buf_gather_max: out[i, f] = max over the K slots of feats[idx[i, k], f], a shadow (idx >= ns) reading as a row of zeros."""
    feats = _a(feats, dtype)
    ns = feats.shape[0]
    f_pad = np.concatenate([feats, np.zeros((1, feats.shape[1]), dtype)])
    return f_pad[np.minimum(np.asarray(idx), ns)].max(1)


def vn_std(x, z, dtype=np.float64):
    """buf_vn_std: x [n,3c], z [n,9] -> out[i, 3c + k] = sum_j x[i, c, j] * z[i, k, j]."""
    x, z = _a(x, dtype), _a(z, dtype)
    n = x.shape[0]
    return _dot3(x.reshape(n, -1, 1, 3), z.reshape(n, 1, 3, 3)).reshape(n, -1)
