"""Named inputs of the patch-selection tests (tests/test_patches_ref_cpu.py checks the reference on them without a device,
tests/test_patch_select_gpu.py runs the kernels on them).  numpy only.

A case is a batch: `clouds` (list of f32[n_c,3]), `kpts` (list of f32[m,3], one per cloud, the same m), `radius`, `nsamples`
(every patch size the case is run at).  `random` marks cases whose coordinates are drawn at random (the float32 / float64
membership check of the CPU tests runs on those); `lattice` marks the case whose coordinates are multiples of 1/64.
"""
import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

import patches_ref


@dataclass
class Case:
    name: str
    clouds: list
    kpts: list
    radius: float
    nsamples: tuple
    random: bool = True
    lattice: bool = False
    notes: dict = field(default_factory=dict)

    @property
    def m(self):
        return len(self.kpts[0]) if self.kpts else 0

    @property
    def lengths(self):
        return [len(c) for c in self.clouds]

    def stacked(self):
        sup = np.concatenate(self.clouds) if self.clouds else np.zeros((0, 3), np.float32)
        kp = np.concatenate(self.kpts) if self.kpts else np.zeros((0, 3), np.float32)
        return np.ascontiguousarray(sup, np.float32).reshape(-1, 3), np.ascontiguousarray(kp, np.float32).reshape(-1, 3)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def _box_cloud(rng, n, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return _f(lo + rng.random((n, 3)) * (hi - lo))


# ----------------------------------------------------------------------------------------------- a. exact sphere
SPHERE_OFFSETS = ((65, 0, 0), (63, 16, 0), (33, 56, 0), (25, 60, 0), (39, 52, 0))        # |o|^2 = 65^2 each


def sphere_offsets():
    """int[102,3]: every permutation and sign change of SPHERE_OFFSETS"""
    out = set()
    for o in SPHERE_OFFSETS:
        assert sum(v * v for v in o) == 65 * 65
        for p in itertools.permutations(o):
            for s in itertools.product((1, -1), repeat=3):
                out.add(tuple(a * b for a, b in zip(p, s)))
    return np.array(sorted(out), np.int64)


def _one_step_inside(off):
    """the lattice neighbour of each offset one step towards the centre along its longest axis"""
    ins = off.copy()
    ax = np.abs(off).argmax(1)
    rows = np.arange(len(off))
    ins[rows, ax] -= np.sign(off[rows, ax])
    return ins


def exact_sphere():
    """Integer lattice / 64, |coordinate| <= 8, r = 65/64: float32 distances are exact, so membership holds in any precision.
    Around each keypoint 102 points exactly ON its sphere (d2 == r2: excluded by the strict '<') and the 102 lattice
    neighbours one step inside (included), among background lattice points; the cloud's order is shuffled."""
    rng = np.random.default_rng(101)
    off = sphere_offsets()
    ins = _one_step_inside(off)
    clouds, kpts, on, inside = [], [], [], []
    for n_kp, n_bg in ((16, 2500), (5, 700)):
        k = rng.integers(-6 * 64, 6 * 64 + 1, (n_kp, 3))
        planted_on = (k[:, None, :] + off[None]).reshape(-1, 3)
        planted_in = (k[:, None, :] + ins[None]).reshape(-1, 3)
        bg = rng.integers(-8 * 64, 8 * 64 + 1, (n_bg, 3))
        allp = np.concatenate([planted_on, planted_in, bg])
        tag = np.concatenate([np.full(len(planted_on), 1), np.full(len(planted_in), 2), np.zeros(n_bg, np.int64)])
        owner = np.concatenate([np.repeat(np.arange(n_kp), len(off))] * 2 + [np.full(n_bg, -1)])
        order = rng.permutation(len(allp))
        allp, tag, owner = allp[order], tag[order], owner[order]
        assert np.abs(allp).max() <= 8 * 64
        clouds.append(_f(allp / 64.0))
        kpts.append(_f(k / 64.0))
        on.append([np.flatnonzero((tag == 1) & (owner == q)) for q in range(n_kp)])
        inside.append([np.flatnonzero((tag == 2) & (owner == q)) for q in range(n_kp)])
    # the same number of keypoints per cloud: the second cloud's are padded with lattice points of its own
    pad = rng.integers(-6 * 64, 6 * 64 + 1, (len(kpts[0]) - len(kpts[1]), 3))
    kpts[1] = np.concatenate([kpts[1], _f(pad / 64.0)])
    return Case('exact_sphere', clouds, kpts, 65.0 / 64.0, (512, 64), random=False, lattice=True, notes=dict(on=on, inside=inside))


# ----------------------------------------------------------------------------------------------- b. mask seams
SEAM_N = (1, 2, 63, 64, 65, 127, 128, 4095, 4096, 4097, 8191, 8193)
SEAM_M = 5


def _centre(i):
    return np.array([3.0 * (i % 4), 3.0 * (i // 4), -2.0 + 0.5 * i])


def seams_all_hits():
    """Every cloud lies in a 0.1 cube around its own centre and so do its keypoints, r = 0.3: every index is a hit.  nsample - 1 =
    keep falls below, at and above the hit counts and inside a mask word."""
    rng = np.random.default_rng(102)
    clouds, kpts = [], []
    for i, n in enumerate(SEAM_N):
        c = _centre(i)
        clouds.append(_box_cloud(rng, n, c - 0.05, c + 0.05))
        kpts.append(_box_cloud(rng, SEAM_M, c - 0.05, c + 0.05))
    return Case('seams_all_hits', clouds, kpts, 0.3, (1, 2, 3, 64, 65, 71, 512))


def seam_hit_indices(n):
    want = {0, 63, 64, 65, n - 2, n - 1}
    if n > 4096:
        want |= set(range(64, n, 128))                      # the first index of every odd 64-bit word
    return sorted(i for i in want if 0 <= i < n)


def seams_chosen_hits():
    """Only the indices of seam_hit_indices(n) are hits (first and last bit of a word, the last two indices, the first bit of every
    odd word where a lane owns two words); every other point lies 40 radii away."""
    rng = np.random.default_rng(103)
    clouds, kpts = [], []
    for i, n in enumerate(SEAM_N):
        c = _centre(i)
        p = _box_cloud(rng, n, c - 0.05 + [0.0, 0.0, 12.0], c + 0.05 + [0.0, 0.0, 12.0])
        idx = seam_hit_indices(n)
        p[idx] = _box_cloud(rng, len(idx), c - 0.05, c + 0.05)
        clouds.append(p)
        kpts.append(_box_cloud(rng, SEAM_M, c - 0.05, c + 0.05))
    return Case('seams_chosen_hits', clouds, kpts, 0.3, (512, 71, 4))


# ----------------------------------------------------------------------------------------------- c. outside the box, cell edges
OUTSIDE_R = 0.1
BOXES = (((-1.3, 2.7, 0.4), (-0.2, 3.9, 1.3), 3000), ((5.0, -4.0, -0.7), (5.9, -3.2, 0.4), 1777))


def _face_cloud(rng, lo, hi, n, per_face=60):
    """random points in [lo, hi] with per_face points exactly on each of the six faces"""
    p = _box_cloud(rng, n, lo, hi)
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    for f in range(6):
        rows = slice(f * per_face, (f + 1) * per_face)
        p[rows, f % 3] = lo32[f % 3] if f < 3 else hi32[f % 3]
    p = np.clip(p, lo32, hi32)
    return p[rng.permutation(n)]


def outside_offsets(edge):
    r = OUTSIDE_R
    return (0.5 * r, 0.999 * r, 1.001 * r, 1.5 * edge, 2.5 * edge, 10.0 * edge)


def outside_box(edges=None):
    """Keypoints beyond each of the six faces of the cloud's box, straight out from a point ON that face, by 0.5 r and 0.999 r (that
    point is in the ball), 1.001 r (it is not), and 1.5, 2.5 and 10 cell edges (nothing is).  edges: the cell edge of each cloud's
    grid (the build's own rule where the caller has it; r * 1.00001, the uncoarsened edge, otherwise)."""
    rng = np.random.default_rng(104)
    clouds, kpts = [], []
    for ci, (lo, hi, n) in enumerate(BOXES):
        p = _face_cloud(rng, lo, hi, n)
        edge = edges[ci] if edges is not None else OUTSIDE_R * 1.00001
        mn, mx = p.min(0), p.max(0)
        k = []
        for f in range(6):
            ax, val, sgn = f % 3, (mn if f < 3 else mx)[f % 3], (-1.0 if f < 3 else 1.0)
            on_face = np.flatnonzero(p[:, ax] == val)
            assert len(on_face) >= 6
            for j, d in enumerate(outside_offsets(edge)):
                q = p[on_face[j]].astype(np.float64)
                q[ax] += sgn * d
                k.append(q)
        clouds.append(p)
        kpts.append(_f(np.array(k)))
    return Case('outside_box', clouds, kpts, OUTSIDE_R, (512, 8))


def cell_edges(edges=None, dims=None):
    """Keypoints whose coordinate along one axis is mn + j * edge rounded to float32, and its two float32 neighbours, for j at both
    ends of the grid and inside it: the query's cell must be the one the build put the points of that slab in."""
    rng = np.random.default_rng(105)
    clouds, kpts = [], []
    for ci, (lo, hi, n) in enumerate(BOXES):
        p = _face_cloud(rng, lo, hi, n)
        mn, mx = p.min(0), p.max(0)
        edge = edges[ci] if edges is not None else OUTSIDE_R * 1.00001
        dim = dims[ci] if dims is not None else [int(np.floor((float(mx[a]) - float(mn[a])) / edge)) + 1 for a in range(3)]
        k = []
        for ax in range(3):
            for j in (0, 1, 2, dim[ax] - 1, dim[ax]):
                v = np.float32(float(mn[ax]) + j * edge)
                for w in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))):
                    q = p[rng.integers(0, n)].copy()
                    q[ax] = w
                    k.append(q)
        clouds.append(p)
        kpts.append(_f(np.array(k)))
    return Case('cell_edges', clouds, kpts, OUTSIDE_R, (512, 8))


# ----------------------------------------------------------------------------------------------- d. coarsened grid, non-finite data
def coarse_and_nonfinite():
    """r = 0.05.  Cloud 0: 3000 points and one 10 km away (the table no longer fits at the radius: coarsened cells).  Cloud 1: one
    point at 1e30 (squared distances overflow).  Cloud 2: NaN, +inf and -inf at index 0, in the middle and at index n - 1.  Keypoints:
    points of the cloud, the odd point itself, NaN and infinities."""
    rng = np.random.default_rng(106)
    m = 40
    clouds, kpts = [], []
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for ci, n in enumerate((3000, 2500, 2001)):
        lo = np.array([1.0 + 2 * ci, -1.0, 0.25])
        p = _box_cloud(rng, n, lo, lo + 0.4)
        k = p[rng.integers(0, n, m)].copy()
        k[1::2] += rng.normal(0, 0.01, k[1::2].shape).astype(np.float32)
        if ci == 0:
            p[1234] = lo.astype(np.float32) + np.float32(10000.0)
            k[0] = p[1234]
            k[1] = p[1234] + np.float32(0.01)
        elif ci == 1:
            p[77] = (np.float32(1e30), p[77, 1], p[77, 2])
            k[0] = p[77]
            k[1] = (np.float32(-1e30), np.float32(1e30), np.float32(0))
        else:
            p[0] = (nan, p[0, 1], p[0, 2])
            p[n // 2] = (inf, inf, inf)
            p[n - 1] = (p[n - 1, 0], -inf, p[n - 1, 2])
            k[0] = (nan, nan, nan)
            k[1] = (k[1, 0], nan, k[1, 2])
            k[2] = (inf, inf, inf)
            k[3] = (k[3, 0], k[3, 1], -inf)
            k[4] = p[1] + np.float32(9.0)                 # empty ball: slot 0 is point 0, the NaN row
        clouds.append(p)
        kpts.append(_f(k))
    return Case('coarse_and_nonfinite', clouds, kpts, 0.05, (512, 16))


# ----------------------------------------------------------------------------------------------- e. batch structure
BATCH_SHAPES = ((1, 0), (1, 1), (1, 5), (1, 9), (3, 5), (4, 5), (3, 9), (5, 9), (6, 1), (8, 1), (9, 1), (15, 1))
# workgroups = nc * ceil(m / 4): 0, 1, 2, 3, 6, 8, 9, 15, 6, 8, 9, 15 -- below, at and above the eight blocks of one remap round


def batch_structure(nc, m, empty=False):
    """nc clouds of different sizes at disjoint places, keypoints from the own cloud (a keypoint held against another cloud finds an
    empty ball there).  From five clouds on, the first, the middle and the last cloud are empty; empty=True: one empty cloud alone."""
    rng = np.random.default_rng(1000 + 16 * nc + m)
    clouds, kpts = [], []
    for c in range(nc):
        n = 300 + 97 * c
        if empty or (nc >= 5 and c in (0, nc // 2, nc - 1)):
            n = 0
        ctr = _centre(c + 1)
        p = _box_cloud(rng, n, ctr - 0.5, ctr + 0.5)
        if n:
            k = p[rng.integers(0, n, m)].copy()
            k[::3] += np.float32(0.02)
        else:
            k = _box_cloud(rng, m, ctr - 0.5, ctr + 0.5)
        clouds.append(p)
        kpts.append(_f(k))
    return Case(f'batch_{nc}x{m}' + ('_empty' if empty else ''), clouds, kpts, 0.3, (32, 2))


# ----------------------------------------------------------------------------------------------- f. large mask
LARGE_N = (98305, 131072, 131073)


def large_mask(n):
    """One cloud in a cube of edge 4 with 16 keypoints, r = 0.3: ~230 hits spread over the whole index range.  98 305 and 131 072 points
    take a mask above 48 KB of LDS for the four waves of a workgroup; 131 073 points have no mask."""
    rng = np.random.default_rng(n)
    p = _box_cloud(rng, n, (0, 0, 0), (4, 4, 4))
    k = p[rng.integers(0, n, 16)].copy()
    k[:2] = p[[0, n - 1]]
    k[8:] += np.float32(0.05)
    return Case(f'large_{n}', [p], [_f(k)], 0.3, (512, 64))


# ----------------------------------------------------------------------------------------------- i. composition
def composition():
    rng = np.random.default_rng(109)
    clouds = [_box_cloud(rng, 3000, (0, 0, 0), (1.5, 1.2, 0.9)), _box_cloud(rng, 3000, (4, 0, 0), (5.0, 1.5, 1.0))]
    kpts = [c[rng.integers(0, len(c), 32)] + np.float32(0.01) for c in clouds]
    return Case('composition', clouds, [_f(k) for k in kpts], 0.3, (512,))


# ----------------------------------------------------------------------------------------------- g. ball query
BQ_N = (1, 63, 64, 65, 129)
BQ_B, BQ_M = 3, 7


def ball_query_case(n):
    """xyz f32[3,n,3], new_xyz f32[3,7,3], r = 0.3.  Query j sits at (5 j, 0, 0); point i of batch element e lies beside query
    (i + e) % 9 (7 and 8: beside nobody).  Query 5 owns only indices from 70 on (its first hit falls in the second 64-block), query 6
    owns nothing (an empty row)."""
    rng = np.random.default_rng(200 + n)
    xyz = np.empty((BQ_B, n, 3), np.float32)
    new = np.zeros((BQ_B, BQ_M, 3), np.float32)
    new[:, :, 0] = 5.0 * np.arange(BQ_M)
    for e in range(BQ_B):
        for i in range(n):
            j = (i + e) % 9
            if j >= 7 or j == 6 or (j == 5 and i < 70):
                ctr = np.array([-20.0, 7.0, 0.0])
            else:
                ctr = np.array([5.0 * j, 0.0, 0.0])
            xyz[e, i] = ctr + rng.uniform(-0.1, 0.1, 3)
    return xyz, new, 0.3


# ----------------------------------------------------------------------------------------------- registry
@functools.lru_cache(maxsize=None)
def get(name):
    if name.startswith('large_'):
        return large_mask(int(name[6:]))
    if name.startswith('batch_'):
        shape = name[6:].replace('_empty', '')
        nc, m = (int(v) for v in shape.split('x'))
        return batch_structure(nc, m, name.endswith('_empty'))
    return {'exact_sphere': exact_sphere, 'seams_all_hits': seams_all_hits, 'seams_chosen_hits': seams_chosen_hits,
            'outside_box': outside_box, 'cell_edges': cell_edges, 'coarse_and_nonfinite': coarse_and_nonfinite,
            'composition': composition}[name]()


BATCH_NAMES = tuple(f'batch_{nc}x{m}' for nc, m in BATCH_SHAPES) + ('batch_1x5_empty',)
LARGE_NAMES = tuple(f'large_{n}' for n in LARGE_N)
SMALL_NAMES = ('exact_sphere', 'seams_all_hits', 'seams_chosen_hits', 'outside_box', 'cell_edges', 'coarse_and_nonfinite', 'composition')
ALL_NAMES = SMALL_NAMES + BATCH_NAMES + LARGE_NAMES


@functools.lru_cache(maxsize=None)
def reference(name, nsample):
    """f32[nc*m, nsample, 3] of the named case, computed once and shared (read-only)"""
    c = get(name)
    sup, kp = c.stacked()
    out = patches_ref.select_patches_batched_ref(sup, c.lengths, kp, c.m, c.radius, nsample)
    out.setflags(write=False)
    return out
