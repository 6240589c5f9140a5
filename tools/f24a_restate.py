#!/usr/bin/env python3
"""The descriptor CNN restated on the CPU in float32 with the summation order of the forms on F(2x4) sets of their own (csrc/convnet_w24a.hip): F(2x4) tiles in
every layer -- the 128-output layers as w24_layer_pair runs them, every 64-output layer (layer 0 included) and the 32-output layers in the
pass-split order of tools/f24p_restate.py (one accumulator set per row component over the whole K, A4^T folded once per row component,
row 0 = (f_0 + f_1) + f_2, row 1 = (f_1 - f_2) - f_3), with the direct round of row 6 summed over the two K halves separately in the
32-output layers.  Against the float64 stack -- the figure the kernel's tests are bounded by (1e-5 of the output scale) -- beside the
order of the pass split in the flagged layers only.

    python tools/f24a_restate.py [patches]

The stacks: the released weights and the two random stacks of tests/test_cyl_f24a_gpu.py.  numpy sums a K range in its own order: the
figure is the size of the rounding error, not a bit pattern."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f24k_restate as k  # noqa: E402
import f24p_restate as p  # noqa: E402
from f24k_restate import f32, pad  # noqa: E402

STACK_A = [48, 64, 32, 32, 64, 64, 64, 32, 32]
STACK_B = [16, 64, 128, 128, 64, 64, 32, 32, 32]


def layer_f24_pass_split32(x, w, b):
    """layer_f24_pass_split with row 6, columns 0..15 as the sum of two K halves (the bias in the lower one)"""
    y = p.layer_f24_pass_split(x, w, b)
    xp = pad(x)
    taps = np.stack([np.stack([xp[:, 6 + a, bb:bb + 16] for bb in range(3)], 1) for a in range(2)], 1)      # [c, a, b, p]
    ks = np.array_split(np.arange(w.shape[1]), 2)
    lo, hi = (np.einsum('ocab,cabp->op', w[:, kk, :2], taps[kk]).astype(f32) for kk in ks)
    y[:, 6, :16] = (lo + b[:, None]).astype(f32) + hi
    return y.astype(f32)


def stack32_all(x, layers):
    h = x.astype(f32)
    for w, b, relu in layers:
        cout = w.shape[0]
        h = k.layer_f24(h, w, b, 1) if cout == 128 else (p.layer_f24_pass_split(h, w, b) if cout == 64 else layer_f24_pass_split32(h, w, b))
        h = np.maximum(h, 0) if relu else h
    return h


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(1)
    stacks = [('stack A ' + '-'.join(map(str, STACK_A)), k.random_stack(STACK_A, 24)), ('stack B ' + '-'.join(map(str, STACK_B)), k.random_stack(STACK_B, 24))]
    rel = k.released_layers()
    if rel is not None:
        stacks.insert(0, ('released weights', [(np.asarray(w, f32), np.asarray(b, f32), r) for w, b, r in rel]))
    for name, layers in stacks:
        for signed in (True, False):
            worst = dict(a=0.0, p=0.0)
            for _ in range(n):
                x = rng.random((layers[0][0].shape[1], 7, 20))
                x = x * 2 - 1 if signed else x
                ref = k.stack64(x, layers)
                worst['a'] = max(worst['a'], np.abs(stack32_all(x, layers) - ref).max() / np.abs(ref).max())
                worst['p'] = max(worst['p'], np.abs(p.stack32_pass_split(x, layers) - ref).max() / np.abs(ref).max())
            print(f'{name}, {"signed" if signed else "non-negative"}, {n} patches: F(2x4) in all layers {worst["a"]:.2e} | flagged layers only {worst["p"]:.2e}')
