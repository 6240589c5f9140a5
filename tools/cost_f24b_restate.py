#!/usr/bin/env python3
"""The two layer forms of csrc/costnet_w24b.hip restated on the CPU in float32, beside those of tools/cost_f24_restate.py:

* layer 1 on F(2x4) tiles in the kernel's summation order: one k' plane (32 of the 96 collapsed input channels) at a time; inside a plane
  each of the four row-component passes starts from cleared accumulators (the bias in column component 1 of pass 1 of plane 0), A4^T is
  folded after each pass into s_I, and the outputs take
      row 0 += s_0;   row 0 += s_1, row 1 += s_1;   row 0 += s_2, row 1 -= s_2;   row 1 -= s_3
  plane after plane.  ('l1-running' is the order of w24_round carried over to planes -- the accumulators run on through the passes, F_I
  is their fold after pass I, row 1 -= F_0, = fma(2, F_1, row 1), row 0 += F_2, row 1 -= F_3 -- which was tried first and is printed for
  comparison: three times the folds of sums that cancel);
* layer 3 as the hybrid: output rows 0..9 from F(2x4) tiles (5 x 3 tiles, windows inside their 14-word rows), rows 10, 11 from the F(2x2)
  tile row 5.

    python tools/cost_f24b_restate.py

prints max |ind - ind64| against the network in float64 for 'all', 'l1', 'l3' and for the parent's forms (those of csrc/costnet_w24.hip: 'off'), on the 40
matches of tests/golden/match_tiny.npz and on 70 random normalised maps (seed 1), released weights.  The kernel's tests bound it by 1e-4
(ind in [0, 20)).  As in the sibling, numpy sums a K range in its own order: the figure is the size of the rounding error, not a bit
pattern."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_f24_restate as r  # noqa: E402

f32 = np.float32


def fma(a, b, c):
    """float32 fma of arrays: one rounding (the float64 product and sum of float32 values are exact to well below half an ulp of the result)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def fold4(acc):
    """A4^T of the six column components acc[j] as w24_round forms it"""
    p, q = acc[1] + acc[2], acc[1] - acc[2]
    t, d = acc[3] + acc[4], acc[3] - acc[4]
    two, four, eight = f32(2), f32(4), f32(8)
    return np.stack([acc[0] + p + t, fma(np.broadcast_to(two, d.shape), d, q), fma(np.broadcast_to(four, t.shape), t, p),
                     fma(np.broadcast_to(eight, d.shape), d, q) + acc[5]], -1)       # [o, ty, tx, v]


def conv_f24_planes(x, w, b, plane=32, running=False):
    """x [C, H, W] with W - 2 a multiple of 4 and H even -> [O, H - 2, W - 2], the channels in planes of `plane`, summed as the docstring
    says; running: w24_round's order instead (the accumulators run on through the passes)"""
    c, h, wd = x.shape
    ny, nx = (h - 2) // 2, (wd - 2) // 4
    assert 4 * nx == wd - 2 and c % plane == 0
    d = np.empty((c, 4, 6, ny, nx), f32)
    for a in range(4):
        for bb in range(6):
            d[:, a, bb] = x[:, a:a + 2 * ny:2, bb:bb + 4 * nx:4]
    v = np.einsum('ia,cabyx,jb->ijcyx', r.BT2, d, r.BT4).astype(f32)
    u = np.einsum('ia,ocab,jb->ijoc', r.G2, w.astype(np.float64), r.G4).astype(f32)
    o = w.shape[0]
    y = np.zeros((2, o, ny, nx, 4), f32)                                         # [output row of the tile][o][ty][tx][v]
    for k in range(c // plane):
        cs = slice(k * plane, (k + 1) * plane)
        acc = np.zeros((6, o, ny, nx), f32)
        for i in range(4):
            part = np.einsum('joc,jcyx->joyx', u[i][:, :, cs], v[i][:, cs]).astype(f32)
            if running:
                if i == 1 and k == 0:
                    acc[1] = acc[1] + b.astype(f32)[:, None, None]
                acc = (acc + part).astype(f32)
                f = fold4(acc)
                if i == 1:
                    y[1] = fma(np.broadcast_to(f32(2), f.shape), f, y[1])
                elif i == 2:
                    y[0] = y[0] + f
                else:
                    y[1] = y[1] - f
                continue
            if i == 1 and k == 0:
                part[1] = part[1] + b.astype(f32)[:, None, None]
            f = fold4(part)
            if i <= 2:
                y[0] = y[0] + f
            if i == 1:
                y[1] = y[1] + f
            if i >= 2:
                y[1] = y[1] - f
    return y.transpose(1, 2, 0, 3, 4).reshape(o, 2 * ny, 4 * nx)


def conv_l3_hybrid(x, w, b):
    """[64, 14, 14] -> [128, 12, 12]: rows 0..9 on F(2x4) tiles, rows 10, 11 on the F(2x2) tile row 5"""
    top = r.conv_f24(x[:, :12], w, b)                                           # tile rows 0..4 read the input rows 0..11
    tail = r.conv_f22(x[:, 10:], w, b)                                          # tile row 5: input rows 10..13
    return np.concatenate([top, tail], 1)


def ind_of(s, t, layers, form):
    """one match; form: 'f64', 'off' (the forms of csrc/costnet_w24.hip), 'all', 'l1', 'l3', 'l1-running'"""
    if form == 'f64':
        return r.ind_of(s, t, layers, 'f64')
    mine = {'off': (), 'all': (1, 3), 'l1': (1,), 'l3': (3,), 'l1-running': (1,)}[form]
    x = r.cost_volume(s, t, f32)
    w0, b0 = layers[0]
    h = np.stack([r.conv_direct(x[:, :, k:k + 3].transpose(0, 2, 1, 3).reshape(96, 20, 20),
                                np.transpose(w0, (0, 1, 3, 2, 4)).reshape(32, 96, 3, 3), b0, f32) for k in range(3)], 1)
    h = np.maximum(h, 0)
    w1, b1 = layers[1]
    x1 = h.transpose(1, 0, 2, 3).reshape(96, 18, 18)
    w1_2d = np.transpose(w1, (0, 3, 1, 2, 4)).reshape(64, 96, 3, 3)
    h = np.maximum(conv_f24_planes(x1, w1_2d, b1, running=form == 'l1-running') if 1 in mine else r.conv_f22(x1, w1_2d, b1), 0)
    for l in range(2, 10):
        w, b = layers[l]
        w2d = w[:, :, :, 0, :]
        if l >= 7:
            y = r.conv_direct(h, w2d, b, f32)
        elif l in (2, 4):
            y = r.conv_f24(h, w2d, b)
        elif l == 3 and 3 in mine:
            y = conv_l3_hybrid(h, w2d, b)
        else:
            y = r.conv_f22(h, w2d, b)
        h = np.maximum(y, 0) if l < 9 else y
    z = h.reshape(-1).astype(f32)
    e = np.exp(z - z.max())
    return float((e * np.arange(20, dtype=f32)).sum() / e.sum())


FORMS = ('all', 'l1', 'l3', 'off')


def errors(se, te, layers, forms=FORMS):
    worst = {f: 0.0 for f in forms}
    for s, t in zip(se, te):
        ref = ind_of(s, t, layers, 'f64')
        for f in forms:
            worst[f] = max(worst[f], abs(ind_of(s, t, layers, f) - ref))
    return worst


if __name__ == '__main__':
    layers = r.released_layers()
    for name, (se, te) in (('match_tiny.npz', r.golden_matches()), ('70 random normalised maps, seed 1', r.random_matches())):
        e = errors(se, te, layers, FORMS + ('l1-running',))
        print(f'{name}, {len(se)} matches: max |ind - ind64|  ' + ' | '.join(f"'{f}' {e[f]:.2e}" for f in e))
