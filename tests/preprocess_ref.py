"""float64 references of the pre-processing kernels (csrc/preprocess.hip) for tests/test_preprocess_edges_gpu.py, and the random inputs that
suite uses (tests/test_preprocess_ref_cpu.py measures the constant K below on exactly these inputs).  Plain numpy, no project code.

Normals: the neighbour set is the brute-force k-NN by (fp64 d2 of the fp32 coordinates, index); the normal is the eigenvector of the
smallest eigenvalue of the population covariance, formed from CENTRED neighbours in np.longdouble and handed to np.linalg.eigh in float64.
The kernel (like open3d) forms the covariance as E[x x^T] - m m^T in fp64: its entries carry an absolute error of the order of
2**-53 (|m|^2 + lambda2), and Davis-Kahan turns that into an angle of the order of that error over the gap lambda1 - lambda0:

    t1 = 2**-53 * (|mean|^2 + lambda2) / (lambda1 - lambda0)            bound_1 = 1.5e-7 + K1 * t1

1.5e-7 = sqrt(3) * 2**-24 rounded up: the fp32 rounding of the three output components.  K1 is measured on the CPU oracle (below).

FINDING (profiles/preprocess_edges.md): t1 does not describe the solver.  In its `half_det >= 0` arm (needles) o3d_fast_eigen3x3 takes
acos of a number within (gap / lambda2)^2 of 1, which loses half the digits: the two small eigenvalues come out with an error of
2**-53 lambda2^2 / gap, and the normal with an angle of the order of

    t2 = 2**-53 * (lambda2 / (lambda1 - lambda0))^2

A needle of length 1 and thickness 1e-3 near the origin is 7e-7 rad off on the host already: K1 measured as prescribed is 5e4, and with
it bound_1 says nothing about a translated cloud (> 1 rad).  The suite therefore asserts the SMALLER of two bounds, either of which
holds for a correct kernel:

    angle_bound = 1.5e-7 + min(K1 * t1, K * (t1 + t2))

K is measured in the same way as K1, as the worst multiple of t1 + t2."""
import functools

import numpy as np

F32_TERM = 1.5e-7
EPS53 = 2.0 ** -53
# Both measured on the CPU by test_preprocess_ref_cpu.py::test_measure_K over every random input of this module (oracle.o3d_estimate_normals
# against normal_ref), never on the device; constant = worst ratio x 8, rounded up to a power of two.
#   K1: worst (angle - 1.5e-7) / t1 = 5.06e4 (needle patches x 1e-4)            -> 2**19
#   K : worst (angle - 1.5e-7) / (t1 + t2) = 0.614 (needle patches translated by (900, -700, 300)) -> 8
K1_MEASURED_WORST, K1 = 5.06e4, 524288.0
K_MEASURED_WORST, K = 0.614, 8.0
BOUND_CAP = 0.05          # a condition on the INPUTS: no random row of the suite may have a larger angle_bound (undetermined normal)


# ------------------------------------------------------------------------------------------------------------------------ references
def knn_sets(pts32, lens, knn):
    """brute force inside each stacked cloud: fp64 d2 of the fp32 coordinates, order (d2, index), min(knn, n_cloud) neighbours with the
    point itself -> list of int64 arrays of GLOBAL indices, nearest first"""
    p = np.asarray(pts32, np.float32).astype(np.float64)
    out, lo = [], 0
    for m in np.asarray(lens, np.int64):
        m = int(m)
        c = p[lo:lo + m]
        k = min(int(knn), m)
        for i0 in range(0, m, 256):
            d = c[None, :, :] - c[i0:i0 + 256, None, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            order = np.argsort(d2, axis=1, kind='stable')[:, :k]           # stable: ties stay in index order
            out.extend(lo + order)
        lo += m
    return out


def rerank(pts32, q, cand, need):
    """the `need` nearest of the DISTINCT candidate indices `cand` to point index q by (fp64 d2, index)"""
    p = np.asarray(pts32, np.float32).astype(np.float64)
    cand = np.asarray(cand, np.int64)
    d = p[cand] - p[q]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return cand[np.lexsort((cand, d2))[:need]]


def normal_ref(pts32, idx_set):
    """-> (n0 f64[3], lambda0, lambda1, lambda2, mean f64[3]) of the population covariance of pts32[idx_set]"""
    x = np.asarray(pts32, np.float32)[np.asarray(idx_set, np.int64)].astype(np.longdouble)
    k = x.shape[0]
    mean = x.sum(0) / k
    c = x - mean
    cov = (c.T @ c) / k
    w, v = np.linalg.eigh(cov.astype(np.float64))
    return v[:, 0].copy(), float(w[0]), float(w[1]), float(w[2]), mean.astype(np.float64)


def bound_terms(lam, mean):
    """(t1, t2) of the module docstring; (inf, inf) when lambda1 == lambda0"""
    l0, l1, l2 = lam
    gap = l1 - l0
    if not gap > 0.0:
        return np.inf, np.inf
    return EPS53 * (float(np.dot(mean, mean)) + l2) / gap, EPS53 * (l2 / gap) ** 2


def angle_bound(lam, mean):
    """lam = (lambda0, lambda1, lambda2) -> rad; inf when lambda1 == lambda0"""
    t1, t2 = bound_terms(lam, mean)
    return F32_TERM + min(K1 * t1, K * (t1 + t2))


def angle(a, b):
    """angle between the LINES spanned by a and b (sign ignored), accurate for small angles"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), abs(float(np.dot(a, b)))))


def det_sign(lam):
    """sign of det(A / max - q I), q = trace / 3, of the solver's shifted matrix: the product of (lambda_i - mean lambda).  < 0 sends
    o3d_fast_eigen3x3 to its `half_det < 0` arm (planar sets), >= 0 to the other (needles)"""
    q = (lam[0] + lam[1] + lam[2]) / 3.0
    return float(np.sign((lam[0] - q) * (lam[1] - q) * (lam[2] - q)))


def voxel_means(pts, voxel, normals=None):
    """open3d voxel_down_sample in numpy: o = min - voxel/2, index = floor((p - o) / voxel), key with N = floor((max - o) / voxel) + 1;
    sequential input-order fp64 sums; rows in ascending key order -> f64[m,3] (, mean normals f64[m,3])"""
    pts = np.asarray(pts, np.float64)
    if pts.shape[0] == 0:
        z = np.zeros((0, 3))
        return z if normals is None else (z, z.copy())
    o = pts.min(0) - voxel * 0.5
    idx = np.floor((pts - o) / voxel).astype(np.int64)
    N = np.floor((pts.max(0) - o) / voxel).astype(np.int64) + 1
    key = idx[:, 0] + N[0] * idx[:, 1] + N[0] * N[1] * idx[:, 2]
    order = np.lexsort((np.arange(len(key)), key))            # by key, input order inside a key
    cols = [pts] if normals is None else [pts, np.asarray(normals, np.float64)]
    rows = [[] for _ in cols]
    lo = 0
    ks = key[order]
    while lo < len(order):
        hi = lo + 1
        while hi < len(order) and ks[hi] == ks[lo]:
            hi += 1
        for a, r in zip(cols, rows):
            s = np.zeros(3)
            for i in order[lo:hi]:                             # input order, sequential fp64 sum
                s = s + a[i]
            r.append(s / (hi - lo))
        lo = hi
    out = [np.array(r) for r in rows]
    return out[0] if normals is None else (out[0], out[1])


def voxel_origin(pts, voxel):
    return np.asarray(pts, np.float64).min(0) - voxel * 0.5


# ---------------------------------------------------------------------------------------------------------------- inputs of the suite
def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def patch_set(kind, seed, rows, k, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """`rows` separate neighbourhoods of k points each (patch r = rows r*k .. r*k+k-1, centres 4 apart) -> f32[rows*k,3].
    plane: a disc of radius 0.5 in a random plane, 2e-3 noise; needle: a segment of length 1 in a random direction, 1e-3 noise;
    edge: two perpendicular half-planes, 1 long and 0.05 wide, 1e-4 noise (lambda0 ~ lambda1 << lambda2)."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rows):
        R = _rot(rng)
        if kind == 'plane':       # stratified in angle and radius: 2 lambda1 > lambda2, the condition of the `half_det < 0` arm
            a, rad = (np.arange(k) + rng.random(k)) * (2 * np.pi / k), 0.5 * np.sqrt((rng.permutation(k) + rng.random(k)) / k)
            loc = np.stack([rad * np.cos(a), rad * np.sin(a), rng.normal(0, 2e-3, k)], 1)
        elif kind == 'needle':
            loc = np.stack([rng.random(k) - 0.5, np.zeros(k), np.zeros(k)], 1) + rng.normal(0, 1e-3, (k, 3))
        elif kind == 'edge':
            w, side = rng.random(k) * 0.05, rng.integers(0, 2, k)
            loc = np.stack([rng.random(k) - 0.5, w * (side == 0), w * (side == 1)], 1) + rng.normal(0, 1e-4, (k, 3))
        else:
            raise ValueError(kind)
        out.append(loc @ R.T + [4.0 * (r % 8), 4.0 * (r // 8), 0.0])
    return (np.concatenate(out) * scale + np.asarray(shift, np.float64)).astype(np.float32)


# name -> (kind, seed, rows, patch size, scale, shift, the knn values used on it) of every random patch set of part (a)
SHIFT = (900.0, -700.0, 300.0)
ZERO = (0.0, 0.0, 0.0)
PATCH_SETS = {
    'plane': ('plane', 11, 16, 30, 1.0, ZERO, (30,)), 'needle': ('needle', 12, 16, 30, 1.0, ZERO, (30,)),
    'edge': ('edge', 13, 16, 30, 1.0, ZERO, (30,)),
    'plane_1e-4': ('plane', 14, 8, 30, 1e-4, ZERO, (30,)), 'plane_1e+3': ('plane', 15, 8, 30, 1e3, ZERO, (30,)),
    'plane_shift': ('plane', 16, 8, 30, 1.0, SHIFT, (30,)),
    'needle_1e-4': ('needle', 17, 8, 30, 1e-4, ZERO, (30,)), 'needle_1e+3': ('needle', 18, 8, 30, 1e3, ZERO, (30,)),
    'needle_shift': ('needle', 19, 8, 30, 1.0, SHIFT, (30,)),
    'plane_nq': ('plane', 20, 129, 30, 1.0, ZERO, (30,)),                       # one patch per row of the nq cases
    'plane_48': ('plane', 21, 4, 48, 1.0, ZERO, (48, 41, 40, 33, 30, 23, 20)),  # the ncand / knn cases and need = ns
}


def patches(name):
    kind, seed, rows, k, scale, shift, _ = PATCH_SETS[name]
    return patch_set(kind, seed, rows, k, scale, shift)


CLOUD_SIZES = (2, 3, 29, 30, 31, 40, 41, 3000)
CLOUD_KINDS = ('mix', 'two_density', 'dup', 'lattice')


def cloud(kind, n, seed=0):
    """the random clouds of part (b), f32[n,3].
    mix: 70 % on a plane patch (3e-3 noise), 30 % on a needle above it (1e-3 noise);
    two_density: a box-corner cloud and a sparse cluster of min(50, n // 2) points 40 m away;
    dup: every point twice (the last one once when n is odd);
    lattice: a shuffled planar lattice (spacing 1/16) with quantised jitter (multiples of 1/512): distances tie exactly in fp32 and fp64."""
    rng = np.random.default_rng(1000 + seed)

    def mix(m):
        npl = m - (3 * m) // 10
        side = 2.0 if m > 100 else 0.3
        pl = np.stack([rng.random(npl) * side, rng.random(npl) * side, rng.normal(0, 3e-3, npl)], 1)
        nd = m - npl
        t = rng.random(nd)
        ne = np.stack([t * side, 0.3 * side + 0.4 * side * t, 0.5 + 0.1 * t], 1) + rng.normal(0, 1e-3, (nd, 3))
        p = np.concatenate([pl, ne])
        return p[rng.permutation(m)] + [0.5, -0.25, 1.0]

    if kind == 'mix':
        p = mix(n)
    elif kind == 'two_density':
        far = min(50, n // 2)
        near = n - far
        face = rng.integers(0, 3, near)
        a = rng.random((near, 3)) * (2.0 if n > 100 else 0.3)
        a[np.arange(near), face] = 0.0
        a += rng.normal(0, 3e-3, a.shape) + 0.5
        b = np.stack([rng.random(far) * 3.0, rng.random(far) * 3.0, rng.normal(0, 0.02, far)], 1) @ _rot(rng).T + 40.0
        p = np.concatenate([b, a])                                   # the far cluster first: rows 0..far-1
    elif kind == 'dup':
        base = mix((n + 1) // 2)
        p = np.repeat(base, 2, axis=0)[:n]
    elif kind == 'lattice':
        side = int(np.ceil(np.sqrt(n))) + 1
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 2)
        g = g[rng.permutation(len(g))[:n]]
        p = np.concatenate([g / 16.0, np.zeros((n, 1))], 1) + rng.integers(-1, 2, (n, 3)) / 512.0 + [1.0, 2.0, 0.5]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=np.float32)


# (cloud kind, n, knn) of every estimate_normals case of part (b) that is compared with normal_ref
def cloud_cases():
    cases = [(kind, n, 30) for kind in CLOUD_KINDS for n in CLOUD_SIZES]
    cases += [('mix', 3000, k) for k in (3, 10, 45)] + [('mix', 41, 45), ('mix', 40, 10)]
    return cases


# rows whose normal is undetermined BY CONSTRUCTION (not by the cap): fewer than 3 neighbours (the kernel answers (0,0,1)), or
# exactly collinear neighbours (('dup', 3): a point, its copy and one more)
def undetermined(kind, n):
    return n < 3 or (kind == 'dup' and n == 3)


# ------------------------------------------------------------------------------------------- references of whole inputs, computed once
def rows_ref(pts32, sets):
    """normal_ref of every row -> (n0 f64[r,3], lam f64[r,3], mean f64[r,3], bound f64[r]); rows of fewer than 3 points: e_z, bound inf"""
    r = len(sets)
    n0, lam, mean, bound = np.zeros((r, 3)), np.zeros((r, 3)), np.zeros((r, 3)), np.full(r, np.inf)
    for i, s in enumerate(sets):
        if len(s) < 3:
            n0[i] = [0.0, 0.0, 1.0]
            continue
        v, l0, l1, l2, m = normal_ref(pts32, s)
        n0[i], lam[i], mean[i] = v, (l0, l1, l2), m
        bound[i] = angle_bound((l0, l1, l2), m)
    return n0, lam, mean, bound


@functools.lru_cache(maxsize=None)
def cloud_reference(kind, n, knn):
    pts = cloud(kind, n)
    sets = knn_sets(pts, [n], knn)
    return (pts, sets) + rows_ref(pts, sets)


@functools.lru_cache(maxsize=None)
def patch_reference(name, knn=None):
    """every point of the set with its knn nearest (default: its whole patch) -> (pts, sets, n0, lam, mean, bound)"""
    pts = patches(name)
    k = PATCH_SETS[name][3]
    sets = knn_sets(pts, [k] * (pts.shape[0] // k), k if knn is None else knn)
    return (pts, sets) + rows_ref(pts, sets)
