"""Plain numpy statements of patch selection (buffer_amd/csrc/pointops.hip: k_select_patches, k_select_patches_grid, k_ball_query,
k_permute_clouds), written from the operators' definitions and independent of the kernels' code paths.  No device, no library.

Membership is the float32 test of `sqdist3`: d2 = dx*dx, then + dy*dy, then + dz*dz, every operation rounded on its own, and
d2 < float32(radius) * float32(radius).  Rows are copied as 32-bit patterns, so NaN payloads and the sign of zero survive.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def sqdist3(q, p):
    """q f32[m,3], p f32[n,3] -> f32[m,n], the operation order of common.h's sqdist3"""
    q, p = _f32(q), _f32(p)
    with np.errstate(all='ignore'):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        r = dx * dx
        r = r + dy * dy
        r = r + dz * dz
    assert r.dtype == np.float32
    return r


def r2_of(radius):
    return np.float32(radius) * np.float32(radius)


def in_ball(pts, kpts, radius):
    """bool[m,n]: point k lies in the ball of keypoint q (NaN and inf distances do not)"""
    with np.errstate(all='ignore'):
        return sqdist3(kpts, pts) < r2_of(radius)


def select_patches_ref(pts, kpts, radius, nsample, hits=None):
    """One cloud: pts f32[n,3], kpts f32[m,3] -> f32[m,nsample,3].  The first nsample-1 hits in index order fill slots 0, 1, ...;
    without a hit slot 0 is point 0 of the cloud (nsample > 1, n > 0); every other slot, and always slot nsample-1, is the keypoint.
    hits: in_ball(pts, kpts, radius) where the caller has it already."""
    pts, kpts = _f32(pts), _f32(kpts)
    n, m = len(pts), len(kpts)
    assert nsample >= 1
    if hits is None:
        hits = in_ball(pts, kpts, radius)
    pb, kb = pts.view(np.uint32), kpts.view(np.uint32)
    out = np.empty((m, nsample, 3), np.uint32)
    for q in range(m):
        idx = np.flatnonzero(hits[q])[:nsample - 1]
        k = len(idx)
        out[q, :k] = pb[idx]
        if k == 0 and nsample > 1 and n > 0:
            out[q, 0] = pb[0]
            k = 1
        out[q, k:] = kb[q]
    return out.view(np.float32)


def select_patches_batched_ref(sup, lengths, kpts, m, radius, nsample):
    """sup f32[sum n_c,3] stacked clouds, kpts f32[nc*m,3] (m keypoints per cloud) -> f32[nc*m,nsample,3]"""
    sup, kpts = _f32(sup), _f32(kpts)
    lengths = [int(v) for v in lengths]
    assert sum(lengths) == len(sup) and len(kpts) == len(lengths) * m
    out = np.empty((len(lengths) * m, nsample, 3), np.float32)
    lo = 0
    for c, n in enumerate(lengths):
        out[c * m:(c + 1) * m] = select_patches_ref(sup[lo:lo + n], kpts[c * m:(c + 1) * m], radius, nsample)
        lo += n
    return out


def ball_query_ref(radius, nsample, xyz, new_xyz):
    """xyz f32[b,n,3], new_xyz f32[b,m,3] -> int32[b,m,nsample]: the first nsample hits in index order, the remaining slots hold the
    first hit, rows without a hit are zero"""
    xyz, new_xyz = np.asarray(xyz, np.float32), np.asarray(new_xyz, np.float32)
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    out = np.zeros((b, m, nsample), np.int32)
    for i in range(b):
        hits = in_ball(xyz[i], new_xyz[i], radius) if n > 0 else np.zeros((m, 0), bool)
        for q in range(m):
            idx = np.flatnonzero(hits[q])[:nsample]
            if len(idx) and nsample > 0:
                out[i, q, :] = idx[0]
                out[i, q, :len(idx)] = idx
    return out


def _prp_hash(x):
    """uint64 array holding 32-bit values -> the same; the 32-bit mixer of prp_hash"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def prp_half_bits(n):
    """the smallest hb >= 1 with 4^hb >= n"""
    hb = 1
    while (1 << (2 * hb)) < n:
        hb += 1
    return hb


def prp_perm(n, key):
    """int64[n] perm with out[j] = src[perm[j]]: a four-round Feistel network on 2*hb bits, keyed by the 64-bit `key` (round rd
    takes the key's bits from 16*rd up, cut to 32, and the constant 0x9e3779b9 * (rd + 1)), applied again until the value falls in [0, n)"""
    n, key = int(n), int(key) & 0xFFFFFFFFFFFFFFFF
    if n == 0:
        return np.zeros(0, np.int64)
    hb = np.uint64(prp_half_bits(n))
    hm = np.uint64((1 << int(hb)) - 1)
    rk = [np.uint64(((key >> (16 * rd)) & 0xFFFFFFFF) ^ ((0x9e3779b9 * (rd + 1)) & 0xFFFFFFFF)) for rd in range(4)]
    v = np.arange(n, dtype=np.uint64)
    todo = np.arange(n)
    while len(todo):
        w = v[todo]
        l, r = w >> hb, w & hm
        for rd in range(4):
            f = _prp_hash(r ^ rk[rd]) & hm
            l, r = r, l ^ f
        w = (l << hb) | r
        v[todo] = w
        todo = todo[w >= np.uint64(n)]
    return v.astype(np.int64)
