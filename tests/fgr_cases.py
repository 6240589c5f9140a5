"""Inputs shared by tests/test_fgr_cpu.py and tests/test_fgr_gpu.py: seeded clouds in the unit cube under a known rigid motion, with
true and false correspondences."""
import functools
import math

import numpy as np


def rigid(rng, angle, t):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def kabsch64(a, b):
    """float64 rigid transform a -> b over corresponding rows"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = cb - T[:3, :3] @ ca
    return T


def errors(T, ref):
    """(rotation error in degrees, translation error) of T against ref"""
    T, ref = np.asarray(T, np.float64), np.asarray(ref, np.float64)
    s = np.linalg.norm(T[:3, :3] - ref[:3, :3]) / (2 * math.sqrt(2))
    return 2 * math.asin(min(1.0, s)) * 180 / math.pi, float(np.linalg.norm(T[:3, 3] - ref[:3, 3]))


@functools.lru_cache(maxsize=None)
def moved_cloud(seed, n, noise=0.0, angle=0.9):
    """-> (src f32[n,3] uniform in the unit cube, tgt f32[n,3] = the moved copy (+ noise), T f64[4,4])"""
    rng = np.random.default_rng(seed)
    src = rng.random((n, 3)).astype(np.float32)
    T = rigid(rng, angle, (0.3, -0.2, 0.5))
    tgt = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    if noise:
        tgt = tgt + rng.normal(scale=noise, size=tgt.shape)
    return src, tgt.astype(np.float32), T


@functools.lru_cache(maxsize=None)
def robust_case(case, variant=False):
    """the robustness case of the issue: 300 points, rows 0..149 true, then false rows matched through a random permutation (150 of
    them; the variant: 300 of them and target noise 0.002) -> (src, tgt, corr int32[n,2], T, seed).  Random false rows largely
    cancel in a least-squares fit, by an amount that varies with the draw: the case takes the first cloud of its seed sequence
    (100 + 10 case, + 1, ...) on which the float64 Kabsch pose over all rows of the plain form is more than 5 degrees off, so that it
    cannot pass without the line process."""
    for k in range(10):
        src, tgt, T = moved_cloud(100 + 10 * case + k, 300, 0.002 if variant else 0.0)
        rng = np.random.default_rng(200 + 10 * case + k)
        true = np.stack([np.arange(150), np.arange(150)], 1)
        plain = np.stack([np.arange(150, 300), rng.permutation(300)[:150]], 1)
        both = np.concatenate([true, plain])
        exact_src, exact_tgt, _ = moved_cloud(100 + 10 * case + k, 300)          # the plain form: no noise
        if errors(kabsch64(exact_src[both[:, 0]], exact_tgt[both[:, 1]]), T)[0] > 5.0:
            break
    else:
        raise AssertionError('no hard input in ten draws')
    false = np.concatenate([plain, np.stack([np.arange(150, 300), rng.permutation(300)[:150]], 1)]) if variant else plain
    return src, tgt, np.concatenate([true, false]).astype(np.int32), T, 11 + case
