#!/usr/bin/env python3
"""The descriptor CNN restated on the CPU in float32 with the summation order of the pass-split form (csrc/convnet_w24p.hip): in the flagged
64-output layers one fresh accumulator set per row component I over the whole K (the bias starts in column component 1 of I = 1), A4^T
folded once per row component, then  row 0 = (f_0 + f_1) + f_2,  row 1 = (f_1 - f_2) - f_3;  the 128-output layers as w24_layer_pair runs
them (the accumulators run on through the passes), F(2x2) elsewhere.  Against the float64 stack -- the figure the kernel's tests are
bounded by (1e-5 of the output scale) -- beside the K-split order of tools/f24k_restate.py.

    python tools/f24p_restate.py [patches]

The stacks: the released weights and the random second stack of tests/test_cyl_f24p_gpu.py (32 -> 64, 128, 128, 64, 64, 32, 32, 32).
numpy sums a K range in its own order: the figure is the size of the rounding error, not a bit pattern."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f24k_restate as k  # noqa: E402
from f24k_restate import A4T, B2T, B4T, f32, ops, pad, untile  # noqa: E402


def layer_f24_pass_split(x, w, b):
    cout, cin = w.shape[:2]
    U = untile(ops.winograd_f24_tile_weights(w), cout, cin)                      # fp32 [4, 6, Cout, Cin]
    xp = pad(x)
    b2, b4, a4 = B2T.astype(f32), B4T.astype(f32), A4T.astype(f32)
    y = np.zeros((cout, 8, 20), f32)
    for ty in range(4):
        for tx in range(5):
            d = xp[:, 2 * ty:2 * ty + 4, 4 * tx:4 * tx + 6]
            V = np.einsum('ia,cab,jb->ijc', b2, d, b4).astype(f32)
            M = np.einsum('ijoc,ijc->ijo', U, V).astype(f32)                     # [i, j, o]: one accumulator set per row component
            M[1, 1] += b                                                         # (the kernel starts that accumulator at the bias)
            f = np.einsum('ijo,vj->iov', M, a4).astype(f32)                      # folded once per row component
            y[:, 2 * ty, 4 * tx:4 * tx + 4] = (f[0] + f[1]) + f[2]
            y[:, 2 * ty + 1, 4 * tx:4 * tx + 4] = (f[1] - f[2]) - f[3]
    y = y[:, :7]
    # row 6, columns 0..15: the direct two-row form over the whole K
    r6 = np.einsum('ocab,cabp->op', w[:, :, :2], np.stack([np.stack([xp[:, 6 + a, bb:bb + 16] for bb in range(3)], 1) for a in range(2)], 1)).astype(f32)
    y[:, 6, :16] = r6 + b[:, None]
    return y.astype(f32)


def stack32_pass_split(x, layers):
    h = x.astype(f32)
    for w, b, relu in layers:
        cout, cin = w.shape[:2]
        if cout == 128:
            h = k.layer_f24(h, w, b, 1)
        elif cout == 64 and cin % 64 == 0:
            h = layer_f24_pass_split(h, w, b)
        else:
            h = k.layer_f22(h, w, b, 2 if cout == 32 else 1)
        h = np.maximum(h, 0) if relu else h
    return h


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(1)
    stacks = [('second stack 32-64-128-128-64-64-32-32-32', k.random_stack([32, 64, 128, 128, 64, 64, 32, 32, 32], 24))]
    rel = k.released_layers()
    if rel is not None:
        stacks.insert(0, ('released weights', [(np.asarray(w, f32), np.asarray(b, f32), r) for w, b, r in rel]))
    for name, layers in stacks:
        for signed in (True, False):
            worst = dict(p=0.0, k=0.0)
            for _ in range(n):
                x = rng.random((layers[0][0].shape[1], 7, 20))
                x = x * 2 - 1 if signed else x
                ref = k.stack64(x, layers)
                worst['p'] = max(worst['p'], np.abs(stack32_pass_split(x, layers) - ref).max() / np.abs(ref).max())
                worst['k'] = max(worst['k'], np.abs(k.stack32(x, layers, True) - ref).max() / np.abs(ref).max())
            print(f'{name}, {"signed" if signed else "non-negative"}, {n} patches: pass split {worst["p"]:.2e} | K split {worst["k"]:.2e}')
