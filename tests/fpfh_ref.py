"""TEST INFRASTRUCTURE: float64 restatement of the FPFH contract of include/buffer_hip.h (N6), in plain Python loops on Python floats
(IEEE fp64, no fused operations), with integer counts.  tests/test_fpfh_cpu.py pins it on hand cases; the GPU tests compare
buf_fpfh with it.

    radius_rows(pts, radius, k, lengths)   the neighbour rows buf_grid_query gives (fp32 d2, ascending by (d2, index), padded with n)
    fpfh(pts, normals, nbr, max_nn)        -> (spfh f64[n,33], fpfh f64[n,33], margin)
    match(fa, fb, mutual)                  numpy twin of buffer_amd.fpfh.match
"""
import math

import numpy as np

NB = 11
DIM = 33


def radius_rows(pts, radius, k, lengths=None):
    """int32[n,k]: per point the <= k nearest points of its own cloud with fp32 d2 = (dx*dx + dy*dy) + dz*dz < radius^2 (fp32),
    itself included, ascending by (d2, index), padded with n"""
    p = np.asarray(pts, np.float32)
    n = len(p)
    lens = [n] if lengths is None else list(lengths)
    out = np.full((n, k), n, np.int32)
    r2 = np.float32(radius) * np.float32(radius)
    lo = 0
    for m in lens:
        q = p[lo:lo + m]
        d = q[:, None, :] - q[None, :, :]
        sq = d * d
        d2 = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)
        for i in range(m):
            hit = np.flatnonzero(d2[i] < r2)
            hit = hit[np.lexsort((hit, d2[i][hit]))][:k]
            out[lo + i, :len(hit)] = hit + lo
        lo += m
    return out


def _bin(x):
    if not (x >= 0.0):
        return 0
    if x >= float(NB):
        return NB - 1
    return int(x)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def pair_feature(pi, ni, pj, nj):
    """(f0, f1, f2) of the pair; arguments are 3-tuples of Python floats"""
    d = (pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2])
    L = math.sqrt(_dot(d, d))
    if L == 0.0:
        return 0.0, 0.0, 0.0
    a1, a2 = _dot(ni, d) / L, _dot(nj, d) / L
    if abs(a1) < abs(a2):
        n1, n2, d, f2 = nj, ni, (-d[0], -d[1], -d[2]), -a2
    else:
        n1, n2, f2 = ni, nj, a1
    v = _cross(d, n1)
    vn = math.sqrt(_dot(v, v))
    if vn == 0.0:
        return 0.0, 0.0, 0.0
    v = (v[0] / vn, v[1] / vn, v[2] / vn)
    w = _cross(n1, v)
    f1 = _dot(v, n2)
    y, x = _dot(w, n2), _dot(n1, n2)
    f0 = float('nan') if (math.isnan(y) or math.isnan(x)) else math.atan2(y, x)
    return f0, f1, f2


def bin_coordinates(f):
    return (11.0 * (f[0] + math.pi) / (2.0 * math.pi), 11.0 * (f[1] + 1.0) / 2.0, 11.0 * (f[2] + 1.0) / 2.0)


def _row(nbr_row, n, kmax):
    """(m_i, the columns 1.. that hold a point)"""
    cols = [c for c in range(kmax) if 0 <= int(nbr_row[c]) < n]
    return len(cols), [c for c in cols if c > 0]


def fpfh(pts, normals, nbr, max_nn):
    """-> (spfh, fpfh, margin); margin = the smallest distance, in bin units, of any unclamped bin coordinate (0 <= x < 11) to an
    integer, over all pairs (inf without one)"""
    P = [tuple(float(v) for v in r) for r in np.asarray(pts, np.float32)]
    N = [tuple(float(v) for v in r) for r in np.asarray(normals, np.float32)]
    nbr = np.asarray(nbr)
    n = len(P)
    kmax = min(int(max_nn), nbr.shape[1]) if n else 0
    counts = np.zeros((n, DIM), np.int64)
    m = np.zeros(n, np.int64)
    margin = float('inf')
    for i in range(n):
        m[i], cols = _row(nbr[i], n, kmax)
        for c in cols:
            j = int(nbr[i, c])
            x = bin_coordinates(pair_feature(P[i], N[i], P[j], N[j]))
            for a in range(3):
                counts[i, NB * a + _bin(x[a])] += 1
                if 0.0 <= x[a] < float(NB):
                    margin = min(margin, abs(x[a] - round(x[a])))
    spfh = np.zeros((n, DIM), np.float64)
    for i in range(n):
        if m[i] >= 2:
            scale = 100.0 / float(m[i] - 1)
            for s in range(DIM):
                spfh[i, s] = float(counts[i, s]) * scale
    out = np.zeros((n, DIM), np.float64)
    for i in range(n):
        if m[i] < 2:
            continue
        acc = [0.0] * DIM
        for c in _row(nbr[i], n, kmax)[1]:
            j = int(nbr[i, c])
            d = (P[j][0] - P[i][0], P[j][1] - P[i][1], P[j][2] - P[i][2])
            d2 = _dot(d, d)
            if not (0.0 < d2 < float('inf')):
                continue
            w = 1.0 / d2
            row = spfh[j]
            for s in range(DIM):
                acc[s] += float(row[s]) * w
        for b in range(3):
            S = 0.0
            for s in range(NB * b, NB * b + NB):
                S += acc[s]
            if S != 0.0:
                f = 100.0 / S
                for s in range(NB * b, NB * b + NB):
                    acc[s] *= f
        for s in range(DIM):
            out[i, s] = acc[s] + spfh[i, s]
    return spfh, out, margin


def match(fa, fb, mutual=True):
    """numpy twin of buffer_amd.fpfh.match: int32[m,2] rows (i, nearest row of fb to fa[i]) on the fp32 casts, ties to the lowest
    row; mutual keeps the rows whose i is the nearest row of fa to fb[j]"""
    a, b = np.asarray(fa, np.float32).astype(np.float64), np.asarray(fb, np.float32).astype(np.float64)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((0, 2), np.int32)
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)
    ab, ba = d.argmin(1), d.argmin(0)
    i = np.arange(len(a))
    if mutual:
        i = i[ba[ab] == i]
    return np.stack([i, ab[i]], 1).astype(np.int32)
