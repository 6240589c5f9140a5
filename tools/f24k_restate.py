#!/usr/bin/env python3
"""The descriptor CNN restated on the CPU in float32 with the arithmetic of k_cyl_net_w24k (csrc/convnet_w24k.hip): F(2x4, 3x3) tiles
in the five flagged layers of the released stack (the K halves of the flagged 64-output layers summed separately, then added), F(2x2)
tiles elsewhere, against the float64 stack -- the figure the kernel's tests are bounded by (1e-5 of the output scale).

    python tools/f24k_restate.py [patches]

Rows 0..5 and row 6, columns 16..19 of a flagged layer come from the F(2x4) tiles, row 6, columns 0..15 from the two-row direct form;
the filter sets are those the kernel streams (fp64 transform rounded once to fp32).  numpy sums a K range in its own order: the figure is
the size of the rounding error, not a bit pattern."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_winograd_f24_cpu import A2T, A4T, B2T, B4T, correlate, untile  # noqa: E402

from buffer_amd import ops  # noqa: E402

f32 = np.float32
G22 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)


def pad(x):
    """[Cin, 7, 20] -> [Cin, 10, 22]: circular azimuth, a zero row above, two below (the eighth output row is dropped)"""
    xp = np.zeros((x.shape[0], 10, 22), x.dtype)
    xp[:, 1:8, 1:21] = x
    xp[:, 1:8, 0], xp[:, 1:8, 21] = x[:, :, 19], x[:, :, 0]
    return xp


def layer_f24(x, w, b, halves):
    cout, cin = w.shape[:2]
    U = untile(ops.winograd_f24_tile_weights(w), cout, cin)                      # fp32 [4, 6, Cout, Cin]
    xp = pad(x)
    b2, b4, a2, a4 = B2T.astype(f32), B4T.astype(f32), A2T.astype(f32), A4T.astype(f32)
    y = np.zeros((cout, 8, 20), f32)
    ks = np.array_split(np.arange(cin), halves)
    for ty in range(4):
        for tx in range(5):
            d = xp[:, 2 * ty:2 * ty + 4, 4 * tx:4 * tx + 6]
            V = np.einsum('ia,cab,jb->ijc', b2, d, b4).astype(f32)
            M = sum(np.einsum('ijoc,ijc->ijo', U[..., k], V[..., k]).astype(f32) for k in ks)
            y[:, 2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4] = np.einsum('ui,ijo,vj->ouv', a2, M, a4)
    y = y[:, :7] + b[:, None, None]
    # row 6, columns 0..15: the direct two-row form
    r6 = sum(np.einsum('ocab,cabp->op', w[:, k, :2], np.stack([np.stack([xp[k, 6 + a, bb:bb + 16] for bb in range(3)], 1) for a in range(2)], 1)).astype(f32)
             for k in ks)
    y[:, 6, :16] = r6 + b[:, None]
    return y.astype(f32)


def layer_f22(x, w, b, halves):
    cout, cin = w.shape[:2]
    U = np.einsum('ia,ocab,jb->ijoc', G22, w.astype(np.float64), G22).astype(f32)
    xp = pad(x)
    b2, a2 = B2T.astype(f32), A2T.astype(f32)
    y = np.zeros((cout, 8, 20), f32)
    ks = np.array_split(np.arange(cin), halves)
    for ty in range(4):
        for tx in range(10):
            d = xp[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]
            V = np.einsum('ia,cab,jb->ijc', b2, d, b2).astype(f32)
            M = sum(np.einsum('ijoc,ijc->ijo', U[..., k], V[..., k]).astype(f32) for k in ks)
            y[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = np.einsum('ui,ijo,vj->ouv', a2, M, a2)
    return (y[:, :7] + b[:, None, None]).astype(f32)


def stack32(x, layers, f24k):
    h = x.astype(f32)
    for w, b, relu in layers:
        cout, cin = w.shape[:2]
        if cout == 128:
            h = layer_f24(h, w, b, 1)
        elif f24k and cout == 64 and cin % 64 == 0:
            h = layer_f24(h, w, b, 2)
        else:
            h = layer_f22(h, w, b, 2 if cout == 32 else 1)
        h = np.maximum(h, 0) if relu else h
    return h


def stack64(x, layers):
    h = x.astype(np.float64)
    for w, b, relu in layers:
        h = correlate(h, w.astype(np.float64)) + b.astype(np.float64)[:, None, None]
        h = np.maximum(h, 0) if relu else h
    return h


def random_stack(widths, seed):
    rng = np.random.default_rng(seed)
    out = []
    for l in range(8):
        cin, cout = widths[l], widths[l + 1]
        out.append(((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(f32), (rng.standard_normal(cout) * 0.1).astype(f32), l < 7))
    return out


def released_layers():
    import torch
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    from buffer_amd.weights import load_weights
    try:
        pe = PatchEmbedder(load_weights('3dmatch'), torch.device('cpu'), THREEDMATCH)
        return pe.layers
    except Exception as e:                                                        # (the embedder wants its device library)
        print('released weights not available here:', e)
        return None


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(1)
    stacks = [('second stack 32-128-128-64-64-32-32-32-32', random_stack([32, 128, 128, 64, 64, 32, 32, 32, 32], 24))]
    rel = released_layers()
    if rel is not None:
        stacks.insert(0, ('released weights', [(np.asarray(w, f32), np.asarray(b, f32), r) for w, b, r in rel]))
    for name, layers in stacks:
        for signed in (True, False):
            worst = {True: 0.0, False: 0.0}
            for _ in range(n):
                x = rng.random((layers[0][0].shape[1], 7, 20))
                x = x * 2 - 1 if signed else x
                ref = stack64(x, layers)
                for f24k in (True, False):
                    worst[f24k] = max(worst[f24k], np.abs(stack32(x, layers, f24k) - ref).max() / np.abs(ref).max())
            print(f'{name}, {"signed" if signed else "non-negative"}, {n} patches: F(2x4) in five layers {worst[True]:.2e} | in the 128-output layers only {worst[False]:.2e}')
