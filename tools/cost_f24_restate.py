#!/usr/bin/env python3
"""The cost net restated on the CPU in float32 with the arithmetic of the layer forms of csrc/costnet_w24.hip: F(2x4, 3x3) tiles in layers 2
and 4 -- the last tile column's window fed from the first two words of the NEXT map row (zeros behind the last row), as the kernel reads
them -- and the Winograd F(2x2) form in layer 6, beside the parent's order (the first forms: F(2x2) in layers 1..5, layer 6 direct).  Both
against the network in float64, on the matches of tests/golden/match_tiny.npz and on 70 random normalised maps (seed 1, as in
tests/test_model_gpu.py::test_fused_cost_volume_vs_library_convs):

    python tools/cost_f24_restate.py

prints max |ind - ind64| of the two forms and their ratio.  The kernel's tests bound it by 1e-4 (ind in [0, 20)).  Every transform
(B^T d B, G g G^T rounded once from float64, A^T m A) and every component GEMM is float32; numpy sums a K range in its own order, and layer
0 is the dense float32 convolution, not the separated form: the figure is the size of the rounding error, not a bit pattern."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32

G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
G4 = np.array([[.25, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], f32)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], f32)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], f32)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], f32)


def conv_direct(x, w, b, dt):
    """valid correlation, x [C, H, W], w [O, C, kh, kw]: one sum over (c, a, b) in dt"""
    kh, kw = w.shape[2:]
    ho, wo = x.shape[1] - kh + 1, x.shape[2] - kw + 1
    win = np.stack([np.stack([x[:, a:a + ho, bb:bb + wo] for bb in range(kw)], 1) for a in range(kh)], 1).astype(dt)      # [c, a, b, y, x]
    return (np.einsum('ocab,cabyx->oyx', w.astype(dt), win, optimize=True).astype(dt) + b.astype(dt)[:, None, None]).astype(dt)


def conv_f22(x, w, b):
    """F(2x2, 3x3) in float32: x [C, H, W] with H, W even -> [O, H - 2, W - 2]"""
    c, h, wd = x.shape
    ny, nx = (h - 2) // 2, (wd - 2) // 2
    d = np.stack([np.stack([x[:, a:a + 2 * ny:2, bb:bb + 2 * nx:2] for bb in range(4)], 1) for a in range(4)], 1).astype(f32)   # [c, a, b, ty, tx]
    v = np.einsum('ia,cabyx,jb->ijcyx', BT2, d, BT2).astype(f32)
    u = np.einsum('ia,ocab,jb->ijoc', G2, w.astype(np.float64), G2).astype(f32)
    m = np.einsum('ijoc,ijcyx->ijoyx', u, v).astype(f32)
    y = np.einsum('ui,ijoyx,vj->oyuxv', AT2, m, AT2).astype(f32).reshape(w.shape[0], 2 * ny, 2 * nx)
    return (y + b.astype(f32)[:, None, None]).astype(f32)


def conv_f24(x, w, b):
    """F(2x4, 3x3) in float32 over the flat channel-major map as cw24_layer reads it: x [C, H, W] (H even) -> [O, H - 2, W - 2].  The
    window of tile (ty, tx) is 4 rows x 6 words from column 4 tx; words past the row's end are the next row's first ones (zeros behind the
    last row) and only meet output columns >= W - 2, which are dropped."""
    c, h, wd = x.shape
    ny, nx = (h - 2) // 2, (wd - 2 + 3) // 4
    flat = np.concatenate([x.reshape(c, h * wd).astype(f32), np.zeros((c, 16), f32)], 1)
    d = np.empty((c, 4, 6, ny, nx), f32)
    for ty in range(ny):
        for tx in range(nx):
            for a in range(4):
                s = (2 * ty + a) * wd + 4 * tx
                d[:, a, :, ty, tx] = flat[:, s:s + 6]
    v = np.einsum('ia,cabyx,jb->ijcyx', BT2, d, BT4).astype(f32)
    u = np.einsum('ia,ocab,jb->ijoc', G2, w.astype(np.float64), G4).astype(f32)
    m = np.einsum('ijoc,ijcyx->ijoyx', u, v).astype(f32)
    y = np.einsum('ui,ijoyx,vj->oyuxv', AT2, m, AT4).astype(f32).reshape(w.shape[0], 2 * ny, 4 * nx)[:, :, :wd - 2]
    return (y + b.astype(f32)[:, None, None]).astype(f32)


def cost_volume(s, t, dt):
    """s, t [32, 5, 20] -> [32, 20 (n), 5 (k), 20 (l)]: S[c][k][(l - n) mod 20] - T[c][k][l]"""
    n, l = np.arange(20)[:, None], np.arange(20)[None, :]
    return (s.astype(dt)[:, :, (l - n) % 20].transpose(0, 2, 1, 3) - t.astype(dt)[:, None]).astype(dt)


def ind_of(s, t, layers, form):
    """one match; form: 'f64' (the network in float64), 'parent' (the first forms in float32), 'new' (those of csrc/costnet_w24.hip), or a tuple of
    the layers (2, 4, 6) that take the new form"""
    dt = np.float64 if form == 'f64' else f32
    new = {'f64': (), 'parent': (), 'new': (2, 4, 6)}.get(form, form)
    x = cost_volume(s, t, dt)                                                   # [c, n, k, l]
    w0, b0 = layers[0]
    # layer 0: 3 x 3 x 3 over (n, k, l) -> [32, 18, 3, 18]; as a 2-d correlation over (n, l) per output k' with channels (c, dk)
    h = np.stack([conv_direct(x[:, :, k:k + 3].transpose(0, 2, 1, 3).reshape(96, 20, 20),
                              np.transpose(w0, (0, 1, 3, 2, 4)).reshape(32, 96, 3, 3), b0, dt) for k in range(3)], 1)       # [o, k', n', l']
    h = np.maximum(h, 0)
    w1, b1 = layers[1]                                                          # collapses k' (3 -> 1): channels (dk, c)
    x1 = h.transpose(1, 0, 2, 3).reshape(96, 18, 18)
    w1_2d = np.transpose(w1, (0, 3, 1, 2, 4)).reshape(64, 96, 3, 3)
    h = np.maximum(conv_direct(x1, w1_2d, b1, dt) if form == 'f64' else conv_f22(x1, w1_2d, b1), 0)
    for l in range(2, 10):
        w, b = layers[l]
        w2d = w[:, :, :, 0, :]
        if form == 'f64' or l >= 7:
            y = conv_direct(h, w2d, b, dt)
        elif l in (2, 4):
            y = conv_f24(h, w2d, b) if l in new else conv_f22(h, w2d, b)
        elif l == 6:
            y = conv_f22(h, w2d, b) if l in new else conv_direct(h, w2d, b, dt)
        else:
            y = conv_f22(h, w2d, b)
        h = np.maximum(y, 0) if l < 9 else y
    z = h.reshape(-1).astype(dt)
    e = np.exp(z - z.max())
    return float((e * np.arange(20, dtype=dt)).sum() / e.sum())


def released_layers():
    from buffer_amd.patch_embedder import _fold_bn
    from buffer_amd.weights import load_weights
    W = load_weights('3dmatch')
    p = 'Inlier.conv.ops'
    layers = [_fold_bn(W[f'{p}.{i}.weight'], W[f'{p}.{i}.bias'], W[f'{p}.{bn}.running_mean'], W[f'{p}.{bn}.running_var'])
              for i, bn in ((0, 1), (3, 4), (6, 7), (9, 10), (12, 13), (15, 16), (18, 19), (21, 22), (24, 25))]
    layers.append((np.asarray(W[f'{p}.27.weight'], f32), np.asarray(W[f'{p}.27.bias'], f32)))
    return layers


def golden_matches():
    f = np.load(os.path.join(ROOT, 'tests', 'golden', 'match_tiny.npz'))
    return f['src_equi'][f['s_mids']][:, :, 1:6], f['tgt_equi'][f['t_mids']][:, :, 1:6]


def random_matches(m=70, seed=1):
    import torch
    g = torch.Generator(device='cpu').manual_seed(seed)
    a = torch.nn.functional.normalize(torch.rand((m, 32, 5, 20), generator=g), dim=1)
    b = torch.nn.functional.normalize(torch.rand((m, 32, 5, 20), generator=g), dim=1)
    return a.numpy(), b.numpy()


def errors(se, te, layers, forms=('new', 'parent')):
    """max |ind - ind64| per form over the matches"""
    worst = {f: 0.0 for f in forms}
    for s, t in zip(se, te):
        ref = ind_of(s, t, layers, 'f64')
        for f in forms:
            worst[f] = max(worst[f], abs(ind_of(s, t, layers, f) - ref))
    return worst


if __name__ == '__main__':
    layers = released_layers()
    for name, (se, te) in (('match_tiny.npz', golden_matches()), ('70 random normalised maps, seed 1', random_matches())):
        e = errors(se, te, layers)
        print(f'{name}, {len(se)} matches: max |ind - ind64|  k_cost_net_w24 forms {e["new"]:.2e} | k_cost_net forms {e["parent"]:.2e} | '
              f'ratio {e["new"] / max(e["parent"], 1e-30):.2f}')
