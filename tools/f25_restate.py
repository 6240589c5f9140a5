#!/usr/bin/env python3
"""The descriptor CNN restated on the CPU in float32 with the summation order of the F(2x5) forms (csrc/convnet_w25.hip): F(2x5, 3x3) tiles
of 2 rows x 5 azimuth columns (4 x 4 tiles carry the 7 x 20 map, the eighth row dropped) in the layers of the chosen output widths, in
the pass-split order -- one fresh accumulator set per row component I over the whole K (the bias starts in the column component of
point +1 of I = 1), A5^T folded once per row component, then  row 0 = (f_0 + f_1) + f_2,  row 1 = (f_1 - f_2) - f_3  -- and the order of
the F(2x4) forms (tools/f24a_restate.py) in every other layer.  Against the float64 stack -- the figure the kernel's tests are bounded by
(1e-5 of the output scale) -- beside the parent order, F(2x4) in all layers.

    python tools/f25_restate.py [patches] [point set ...]

Point sets: 'h' = 0, +-1, +-2, +-1/2 (ops.F25_POINTS, what the kernel runs); others are given as comma-separated points with 'inf' for
the point at infinity, e.g. 0,1,-1,2,-2,-0.5,inf.  The rule of the kernel's issue: F(2x5) in every flagged layer stays within twice the
parent order's figure and below 1e-5.

The stacks: the released weights and the two random stacks of tests/test_cyl_f24a_gpu.py.  numpy sums a K range in its own order: the
figure is the size of the rounding error, not a bit pattern."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f24a_restate as a  # noqa: E402
import f24k_restate as k  # noqa: E402
import f24p_restate as p  # noqa: E402
from f24k_restate import B2T, f32, ops, pad  # noqa: E402


def matrices(points):
    """(B^T [7, 7], G [7, 3], A^T [5, 7]) of F(5, 3) on seven points, float64; 'inf' may be one of them (Toom-Cook with the point at
    infinity: its row of B^T is the monic polynomial through all finite points)"""
    fin = np.array([q for q in points if q != 'inf'], np.float64)
    n = len(points)
    assert n == 7 and len(fin) >= 6
    bt, g, at = np.zeros((n, n)), np.zeros((n, 3)), np.zeros((5, n))
    j = 0
    for col, q in enumerate(points):
        if q == 'inf':
            bt[col, :len(fin) + 1] = np.poly(fin)[::-1]
            g[col, 2] = 1
            at[4, col] = 1
            continue
        lj = np.poly(np.delete(fin, j))[::-1]
        bt[col, :len(lj)] = lj
        g[col] = fin[j] ** np.arange(3) / np.polyval(lj[::-1], fin[j])
        at[:, col] = fin[j] ** np.arange(5)
        j += 1
    return bt, g, at


def check_identity(bt, g, at):
    rng = np.random.default_rng(0)
    d, f = rng.standard_normal(7), rng.standard_normal(3)
    want = np.array([np.dot(d[i:i + 3], f) for i in range(5)])
    got = at @ ((g @ f) * (bt @ d))
    assert np.abs(got - want).max() < 1e-10, (got, want)


def layer_f25(x, w, b, mats):
    bt, g, at = mats
    cout, cin = w.shape[:2]
    U = np.einsum('ia,ocab,jb->ijoc', ops.F24_G2, w.astype(np.float64), g).astype(f32)          # fp64, rounded once
    xp = pad(x)
    b2, b5, a5 = B2T.astype(f32), bt.astype(f32), at.astype(f32)
    y = np.zeros((cout, 8, 20), f32)
    plus1 = 1                                                                    # the column component A5^T carries with weight 1
    assert np.all(at[:, plus1] == 1)
    for ty in range(4):
        for tx in range(4):
            d = xp[:, 2 * ty:2 * ty + 4, 5 * tx:5 * tx + 7]
            V = np.einsum('ia,cab,jb->ijc', b2, d, b5).astype(f32)
            M = np.einsum('ijoc,ijc->ijo', U, V).astype(f32)                     # one accumulator set per row component
            M[1, plus1] += b
            f = np.einsum('ijo,vj->iov', M, a5).astype(f32)                      # folded once per row component
            y[:, 2 * ty, 5 * tx:5 * tx + 5] = (f[0] + f[1]) + f[2]
            y[:, 2 * ty + 1, 5 * tx:5 * tx + 5] = (f[1] - f[2]) - f[3]
    return y[:, :7].astype(f32)


def stack32_f25(x, layers, widths, mats):
    h = x.astype(f32)
    for w, b, relu in layers:
        cout = w.shape[0]
        if cout in widths:
            h = layer_f25(h, w, b, mats)
        else:
            h = k.layer_f24(h, w, b, 1) if cout == 128 else (p.layer_f24_pass_split(h, w, b) if cout == 64 else a.layer_f24_pass_split32(h, w, b))
        h = np.maximum(h, 0) if relu else h
    return h


def parse(arg):
    if arg == 'h':
        return list(ops.F25_POINTS)
    return ['inf' if t == 'inf' else float(t) for t in arg.split(',')]


if __name__ == '__main__':
    args = sys.argv[1:]
    n = int(args.pop(0)) if args and args[0].isdigit() else 4
    sets = [(s, matrices(parse(s))) for s in (args or ['h'])]
    for _, m in sets:
        check_identity(*m)
    bt, g, at = matrices(list(ops.F25_POINTS))
    assert np.array_equal(bt, ops.F25_B5T) and np.allclose(g, ops.F25_G5, rtol=1e-15) and np.array_equal(at, ops.F25_A5T)
    rng = np.random.default_rng(1)
    stacks = [('stack A ' + '-'.join(map(str, a.STACK_A)), k.random_stack(a.STACK_A, 24)), ('stack B ' + '-'.join(map(str, a.STACK_B)), k.random_stack(a.STACK_B, 24))]
    rel = k.released_layers()
    if rel is not None:
        stacks.insert(0, ('released weights', [(np.asarray(w, f32), np.asarray(b, f32), r) for w, b, r in rel]))
    parts = [('64+32', (64, 32)), ('64', (64,)), ('32', (32,)), ('all', (128, 64, 32))]
    for name, layers in stacks:
        for signed in (True, False):
            worst = {}
            for _ in range(n):
                x = rng.random((layers[0][0].shape[1], 7, 20))
                x = x * 2 - 1 if signed else x
                ref = k.stack64(x, layers)
                scale = np.abs(ref).max()
                worst['parent'] = max(worst.get('parent', 0.0), np.abs(a.stack32_all(x, layers) - ref).max() / scale)
                for s, m in sets:
                    for pname, widths in parts:
                        key = f'{s} {pname}'
                        worst[key] = max(worst.get(key, 0.0), np.abs(stack32_f25(x, layers, widths, m) - ref).max() / scale)
            print(f'{name}, {"signed" if signed else "non-negative"}, {n} patches: ' + ' | '.join(f'{key} {v:.2e}' for key, v in worst.items()))
