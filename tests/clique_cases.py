"""Inputs shared by tests/test_clique_cpu.py and tests/test_clique_gpu.py, built on sc2_cases' and fgr_cases' seeded clouds (imported,
not edited), and the restatement's results on them (computed once per process)."""
import functools

import numpy as np

import clique_ref
import sc2_cases

THR = sc2_cases.THR                                              # d_thr of every case that does not set its own
SIZES = sc2_cases.SIZES
MARGINS = ('compat', 'gnc', 'g', 'vote', 'vote_gap', 'residual')
# (name, rows, options, inject dead and duplicate rows): every size at the defaults, then the variants on the sizes around the word
# boundaries of the bit rows
EXACT_CASES = [(f'n{n}', n, {}, False) for n in SIZES] + [
    (f'n{n}_{tag}', n, opts, inject) for n in (65, 129, 300) for tag, opts, inject in (
        ('dead_dup', {}, True),
        ('seeds1', dict(max_seeds=1), False),
        ('members3', dict(max_members=3), False),
        ('members16', dict(max_members=16), False),                # K < size
        ('d0.1', dict(d_thr=0.1), False),                          # false rows enter the clique: GNC engaged, bound > clique
        ('d1e-9', dict(d_thr=1e-9), False),                        # no edges: NOTHING
        ('d10', dict(d_thr=10.0), False))]                         # the complete graph: a walk of n members
GNC_ROWS = list(range(40)) + list(range(100, 108))
GNC_OPTS = dict(d_thr=10.0, tim_thr=0.03, refine_iterations=0)
ROBUST = [(t, c) for t in (30, 15) for c in range(4)] + [(6, c) for c in range(6)]


def margins_hold(m):
    return all(m[k] >= 1e-9 for k in MARGINS)


def run_ref(src, tgt, corr, opts):
    o = dict(opts)
    return clique_ref.clique(src, tgt, corr, o.pop('d_thr', THR), **o)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """-> (src, tgt, corr, options, the restatement's result): the first input of the case's seed sequence that meets the margin
    conditions (tests/test_clique_cpu.py asserts that it meets them)"""
    _, n, opts, inject = next(c for c in EXACT_CASES if c[0] == name)
    for attempt in range(5):
        src, tgt, corr = sc2_cases.exact_input(n, inject, attempt)
        want = run_ref(src, tgt, corr, opts)
        if margins_hold(want['margins']):
            return src, tgt, corr, opts, want
    raise AssertionError(f'{name}: no input with the margins in five draws')


@functools.lru_cache(maxsize=None)
def gnc_case():
    """rows 0..39 (true) and 100..107 (false) of low_inlier_case(40, 0) under a threshold that makes the graph complete: the clique
    holds the false rows and only the GNC can tell them apart -> (src, tgt, corr, options, truth, the restatement's result)"""
    src, tgt, corr, T = sc2_cases.low_inlier_case(40, 0)
    corr = np.ascontiguousarray(corr[GNC_ROWS])
    return src, tgt, corr, GNC_OPTS, T, run_ref(src, tgt, corr, GNC_OPTS)


@functools.lru_cache(maxsize=None)
def robust_case(true_rows, case):
    """sc2_cases.low_inlier_case at THR -> (src, tgt, corr, truth, the restatement's result)"""
    src, tgt, corr, T = sc2_cases.low_inlier_case(true_rows, case)
    return src, tgt, corr, T, run_ref(src, tgt, corr, {})


@functools.lru_cache(maxsize=None)
def large_case():
    """sc2_cases.large_case's input (3 000 rows, 20 % false) -> (src, tgt, corr, the restatement's result)"""
    src, tgt, corr, _ = sc2_cases.large_case()
    return src, tgt, corr, run_ref(src, tgt, corr, {})
