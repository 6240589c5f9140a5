"""Inputs shared by tests/test_sc2_cpu.py and tests/test_sc2_gpu.py, built on fgr_cases' seeded clouds (unit cube, known rigid motion,
target noise 0.002), and the restatement's results on them (computed once per process)."""
import functools

import numpy as np

import fgr_cases
import sc2_ref

THR = 0.03                                                       # d_thr = inlier_thr of every case here
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 300)
# (name, rows, options, inject dead and duplicate rows): every size at the defaults, then the other option values on the sizes
# around the word boundaries of the bit rows
EXACT_CASES = [(f'n{n}', n, {}, False) for n in SIZES] + [
    (f'n{n}_{tag}', n, opts, inject) for n in (65, 129, 300) for tag, opts, inject in (
        ('seeds1_k3_nms', dict(max_seeds=1, k1=3, nms_radius=0.1), False),
        ('seeds7_k128', dict(max_seeds=7, k1=128), False),
        ('nms', dict(nms_radius=0.1), False),
        ('dead_dup', {}, True),
        ('dead_dup_nms_k128', dict(nms_radius=0.1, k1=128), True))]


@functools.lru_cache(maxsize=None)
def exact_input(n, inject=False, attempt=0):
    """n rows on a cloud of max(n, 16) points: the first 60 % true (i -> i), the others matched through a random permutation.
    inject: dead rows at 0, 63, 64 and n - 1 (an index past the end, a negative index, a NaN point, an index past the end) and
    rows 10, 70 and n - 3 repeating row 3 -> (src, tgt, corr int32[n,2])"""
    m = max(n, 16)
    src, tgt, _ = fgr_cases.moved_cloud(700 + n + 1000 * attempt, m, 0.002)
    rng = np.random.default_rng(800 + n + 1000 * attempt)
    corr = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    false = np.arange(n) >= int(np.ceil(0.6 * n))
    corr[false, 1] = rng.permutation(m)[:n][false]
    if inject:
        src = src.copy()
        for r in (10, 70, n - 3):
            if 3 < r < n:
                corr[r] = corr[3]
        corr[0] = (0, m)
        if n > 64:
            corr[63] = (-1, 5)
            src[64] = np.nan                                     # (row 64 is the only row on source point 64)
        corr[n - 1] = (m + 5, 0)
    return src, tgt, corr


def margins_hold(m):
    return all(m[k] >= 1e-9 for k in ('compat', 'residual', 'seed', 'nms'))


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """-> (src, tgt, corr, options, the restatement's result): the first input of the case's seed sequence that meets the margin
    conditions (tests/test_sc2_cpu.py asserts that this is the input the GPU tests use and that it meets them)"""
    _, n, opts, inject = next(c for c in EXACT_CASES if c[0] == name)
    for attempt in range(5):
        src, tgt, corr = exact_input(n, inject, attempt)
        want = sc2_ref.sc2(src, tgt, corr, THR, THR, **opts)
        if margins_hold(want['margins']):
            return src, tgt, corr, opts, want
    raise AssertionError(f'{name}: no input with the margins in five draws')


@functools.lru_cache(maxsize=None)
def low_inlier_case(true_rows, case):
    """the low-inlier input of the issue: 300 correspondences on moved_cloud(500 + case, 300, 0.002), rows 0 .. true_rows - 1 true, the
    others matched through default_rng(600 + case).permutation(300) -> (src, tgt, corr, T)"""
    src, tgt, T = fgr_cases.moved_cloud(500 + case, 300, 0.002)
    perm = np.random.default_rng(600 + case).permutation(300)
    corr = np.stack([np.arange(300), np.arange(300)], 1).astype(np.int32)
    corr[true_rows:, 1] = perm[:300 - true_rows]
    return src, tgt, corr, T


@functools.lru_cache(maxsize=None)
def large_case():
    """3 000 rows on a 1 500-point cloud, 20 % false -> (src, tgt, corr, the restatement's result)"""
    for attempt in range(5):
        src, tgt, _ = fgr_cases.moved_cloud(900 + attempt, 1500, 0.002)
        rng = np.random.default_rng(950 + attempt)
        corr = np.stack([np.arange(3000) % 1500, np.arange(3000) % 1500], 1).astype(np.int32)
        bad = rng.random(3000) < 0.2
        corr[bad, 1] = rng.integers(0, 1500, int(bad.sum()))
        want = sc2_ref.sc2(src, tgt, corr, THR, THR)
        if margins_hold(want['margins']):
            return src, tgt, corr, want
    raise AssertionError('large case: no input with the margins in five draws')
