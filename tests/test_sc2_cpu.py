"""The float64 restatement of N8 (tests/sc2_ref.py) pinned on the CPU: hand-computable inputs, statuses, its robustness on the cases
the GPU tests run, the margin conditions of every input that tests/test_sc2_gpu.py compares exactly, and the part of the surface
that needs no device (Sc2Options, exported symbols, the drivers' --estimator)."""
import numpy as np
import pytest

import fgr_cases
import sc2_cases
import sc2_ref

THR = sc2_cases.THR


def _dyadic_pair():
    """6 points with dyadic coordinates and a target that is the source turned a quarter about z and shifted: every distance is the
    same on both sides, exactly"""
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.5], [0.5, 0.25, 1]], np.float32)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.5, -0.25, 2.0])
    return src, (src.astype(np.float64) @ R.T + t).astype(np.float32), R, t


def test_four_true_rows_and_two_false_rows():
    src, tgt, R, t = _dyadic_pair()
    corr = np.array([[0, 0], [1, 1], [2, 2], [3, 3], [4, 0], [5, 2]], np.int32)      # rows 4 and 5 are false
    out = sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, seed_ratio=1.0)
    # the true rows are compatible with each other exactly (e = 0, s = 1), the false rows with nothing but themselves and a row that
    # shares their target point at a distance that happens to agree: none here
    P, Q, live = sc2_ref.rows_of(src, tgt, corr)
    e = np.abs(sc2_ref.distances(P) - sc2_ref.distances(Q))
    assert live.all() and (e[:4, :4] == 0).all()
    C = e <= 0.01
    assert C[:4, :4].all() and C[4:, :4].sum() == 0 and C[4, 5] == 0
    # confidence: the eigenvector iteration of a block of ones (4 x 4) and two isolated rows: 1 on the block, 4^-10 on the others
    assert np.array_equal(out['conf'][:4], np.ones(4)) and np.allclose(out['conf'][4:], 0.25 ** 10, rtol=1e-12)
    assert out['seeds'][:6].tolist() == [0, 1, 2, 3, 4, 5] and (out['seeds'][6:] == -1).all()
    # second-order counts: 4 on the block for its seeds; an isolated row sees only itself
    for r in range(4):
        assert out['counts'][r].tolist() == [4, 4, 4, 4, 0, 0]
    assert out['counts'][4].tolist() == [0, 0, 0, 0, 1, 0] and out['counts'][5].tolist() == [0, 0, 0, 0, 0, 1]
    assert (out['counts'][6:] == -1).all()
    assert out['hyp_counts'][:6].tolist() == [4, 4, 4, 4, -1, -1]                      # a set of one row is no hypothesis
    assert out['info'].tolist() == [sc2_ref.OK, 6, 6, 0, 4, 4] and out['inliers'].tolist() == [1, 1, 1, 1, 0, 0]
    assert np.allclose(out['T'][:3, :3], R, atol=1e-14) and np.allclose(out['T'][:3, 3], t, atol=1e-14)
    # seed_ratio: S = min(max_seeds, max(1, ceil(ratio n)))
    assert sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, seed_ratio=0.2)['info'][2] == 2
    assert sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, seed_ratio=0.01)['info'][2] == 1
    assert sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, seed_ratio=1.0, max_seeds=3)['info'][2] == 3


def test_dead_rows_and_statuses():
    src, tgt, R, t = _dyadic_pair()
    bad = src.copy()
    bad[1, 2] = np.nan
    dead = np.array([[6, 0], [0, -1], [1, 1], [0, 6]], np.int32)                      # past the end, negative, a NaN point, past the end
    out = sc2_ref.sc2(bad, tgt, dead, 0.01, 0.01)
    assert out['info'].tolist() == [sc2_ref.NOTHING, 0, 0, -1, 0, 0] and np.array_equal(out['T'], np.eye(4))
    assert np.isnan(out['conf']).all() and (out['seeds'] == -1).all() and not out['inliers'].any() and (out['counts'] == -1).all()
    empty = sc2_ref.sc2(src, tgt, np.zeros((0, 2), np.int32), 0.01, 0.01)
    assert empty['info'].tolist() == [sc2_ref.NOTHING, 0, 0, -1, 0, 0] and np.array_equal(empty['T'], np.eye(4))
    two = sc2_ref.sc2(src, tgt, np.array([[0, 0], [1, 1]], np.int32), 0.01, 0.01, seed_ratio=1.0)
    assert two['info'].tolist() == [sc2_ref.NOTHING, 2, 2, -1, 0, 0] and two['hyp_counts'][:2].tolist() == [-1, -1]
    # a dead row among live ones: out of every matrix, the others as without it
    corr = np.array([[0, 0], [1, 1], [9, 9], [2, 2], [3, 3]], np.int32)
    out = sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, seed_ratio=1.0)
    assert out['info'].tolist() == [sc2_ref.OK, 4, 4, 0, 4, 4] and out['inliers'].tolist() == [1, 1, 0, 1, 1] and np.isnan(out['conf'][2])
    assert out['counts'][0].tolist() == [4, 4, 0, 4, 4] and 2 not in out['seeds']
    # a winner with fewer than 3 inliers: an inlier distance that nothing meets
    none = sc2_ref.sc2(src, (tgt + np.float32(0.001) * np.arange(18, dtype=np.float32).reshape(6, 3) % 0.004).astype(np.float32),
                       np.stack([np.arange(6), np.arange(6)], 1), 0.05, 1e-7, seed_ratio=1.0)
    assert none['info'][0] == sc2_ref.NOTHING and none['info'][3] >= 0 and none['info'][4] < 3 and np.array_equal(none['T'], np.eye(4))


def test_one_row_repeated_and_k1_above_n():
    src, tgt, R, t = _dyadic_pair()
    same = np.tile(np.array([[4, 4]], np.int32), (7, 1))
    out = sc2_ref.sc2(src, tgt, same, 0.01, 0.01, k1=128)
    # every row is compatible with every row at e = 0: confidence 1, counts 7, a set of all 7 (k1 = 128 > n), H = 0: the identity
    # rotation, the translation q - p
    assert np.array_equal(out['conf'], np.ones(7)) and out['seeds'][:2].tolist() == [0, 1] and out['counts'][0].tolist() == [7] * 7
    assert out['info'].tolist() == [sc2_ref.OK, 7, 2, 0, 7, 7] and out['inliers'].all()
    assert np.allclose(out['T'][:3, :3], np.eye(3)) and np.allclose(out['T'][:3, 3], tgt[4].astype(np.float64) - src[4], atol=1e-15)
    corr = np.stack([np.arange(6), np.arange(6)], 1).astype(np.int32)
    big = sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, k1=128)
    small = sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, k1=6)
    assert big['info'].tolist() == small['info'].tolist() == [sc2_ref.OK, 6, 2, 0, 6, 6] and np.array_equal(big['T'], small['T'])
    three = sc2_ref.sc2(src, tgt, corr, 0.01, 0.01, k1=3, refine_iterations=0)       # the set: columns 0, 1, 2 (ties to the lowest)
    assert three['info'].tolist() == [sc2_ref.OK, 6, 2, 0, 6, 6] and np.allclose(three['T'][:3, :3], R, atol=1e-14)


@pytest.mark.parametrize('case', range(4))
def test_restatement_is_robust(case):
    """the robustness inputs of the GPU file, with its limits: 0.5 degrees and 0.01"""
    for variant in (False, True):
        src, tgt, corr, T, _ = fgr_cases.robust_case(case, variant)
        out = sc2_ref.sc2(src, tgt, corr, THR, THR)
        rre, rte = fgr_cases.errors(out['T'], T)
        print(f'SC2 restatement, robust case {case} variant {variant}: info {out["info"].tolist()}, {rre:.3e} deg, {rte:.3e}')
        assert out['info'][0] == sc2_ref.OK and rre <= 0.5 and rte <= 0.01
    for true_rows in (30, 15):
        src, tgt, corr, T = sc2_cases.low_inlier_case(true_rows, case)
        out = sc2_ref.sc2(src, tgt, corr, THR, THR)
        rre, rte = fgr_cases.errors(out['T'], T)
        plain = fgr_cases.errors(fgr_cases.kabsch64(src[corr[:, 0]], tgt[corr[:, 1]]), T)
        print(f'SC2 restatement, {true_rows} true rows of 300, case {case}: info {out["info"].tolist()}, {rre:.3e} deg, {rte:.3e}; plain '
              f'Kabsch {plain[0]:.2f} deg')
        assert out['info'][0] == sc2_ref.OK and rre <= 0.5 and rte <= 0.01 and plain[0] > 5.0
        assert out['info'][5] >= true_rows and out['inliers'][:true_rows].sum() >= true_rows - 1


@pytest.mark.parametrize('name', [c[0] for c in sc2_cases.EXACT_CASES])
def test_margin_conditions(name):
    """every input that the GPU tests compare exactly: no compatibility, residual or confidence decision within 1e-9 of its threshold.
    An input that violates a condition is replaced by the next draw of its sequence (sc2_cases.exact_case), never excused."""
    src, tgt, corr, opts, want = sc2_cases.exact_case(name)
    m = want['margins']
    print(f'SC2 margins {name}: ' + ', '.join(f'{k} {v:.3e}' for k, v in m.items()))
    assert m['compat'] >= 1e-9 and m['residual'] >= 1e-9 and m['seed'] >= 1e-9 and m['nms'] >= 1e-9
    again = sc2_ref.sc2(src, tgt, corr, THR, THR, **opts)        # the result the GPU test compares with is this input's
    assert np.array_equal(again['info'], want['info']) and np.array_equal(again['counts'], want['counts'])
    if 'nms' in name:
        assert np.isfinite(m['nms'])                             # the suppression had something to compare
    if name in ('n300_nms', 'n300_dead_dup_nms_k128'):           # and, among 300 points, something to suppress
        plain = sc2_ref.sc2(src, tgt, corr, THR, THR, **dict(opts, nms_radius=0.0))
        assert not np.array_equal(plain['seeds'], want['seeds'])


def test_margin_conditions_of_the_larger_input():
    m = sc2_cases.large_case()[3]['margins']
    print('SC2 margins rows3000: ' + ', '.join(f'{k} {v:.3e}' for k, v in m.items()))
    assert m['compat'] >= 1e-9 and m['residual'] >= 1e-9 and m['seed'] >= 1e-9


def test_options_map_onto_the_kernel_arguments():
    from buffer_amd.sc2 import Sc2Options
    o = Sc2Options()
    assert o.kernel_arguments() == dict(d_thr=0.1, inlier_thr=0.1, seed_ratio=0.2, max_seeds=512, k1=30, nms_radius=0.0,
                                        power_iterations=10, refine_iterations=20)
    assert {k: v for k, v in o.kernel_arguments().items() if k not in ('d_thr', 'inlier_thr')} == sc2_ref.DEFAULTS
    k = Sc2Options(d_thr=0.0375, inlier_thr=0.05, k1=40, nms_radius=0.2).kernel_arguments()
    assert (k['d_thr'], k['inlier_thr'], k['k1'], k['nms_radius']) == (0.0375, 0.05, 40, 0.2)
    assert Sc2Options(d_thr=0.0375).inlier_thr == 0.0375 and 'k1=30' in repr(o)


def test_estimator_option(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--estimator', 'sc2'])
        assert a.descriptor == 'fpfh' and a.estimator == 'sc2'
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['--root', 'r', '--estimator', 'sc2'])
        assert e.value.code == 2 and '--descriptor fpfh' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--estimator', 'teaser'])
    from buffer_amd import fpfh
    assert fpfh.ESTIMATORS == ('ransac', 'fgr') and fpfh.ALL_ESTIMATORS == ('ransac', 'fgr', 'sc2')


def test_header_declares_the_entry_points():
    import os
    from buffer_amd import _lib
    assert {'buf_sc2_batched', 'buf_sc2_ws_bytes'} <= set(_lib.exported_symbols())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'buffer_hip.h')).read()
    for word in ('buf_sc2_batched', 'buf_sc2_ws_bytes', 'BUF_SC2_NOTHING', 'BUF_SC2_OK', 'BUF_SC2_MAX_ROWS 16384', 'unpinned'):
        assert word in header, word
