"""Pin tests/pose_ref.py (the float64 references of tests/test_pose_recovery_gpu.py): against fixture match_tiny.npz, which the reference
itself produced, and against oracle/pipeline_ref.ransac_kabsch, the restatement of our sampler.  CPU only."""
import os

import numpy as np

import pose_ref
from oracle import pipeline_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DELTA = 1e-5


def _fixture():
    f = np.load(os.path.join(GOLD, "match_tiny.npz"), allow_pickle=False)
    s, t = f['s_mids'], f['t_mids']
    return f, f['src_kpts'][s], f['tgt_kpts'][t], f['src_R'][s], f['tgt_R'][t]


def test_hypotheses_reproduce_fixture():
    f, ss, tt, ssR, ttR = _fixture()
    R, t = pose_ref.hypotheses(f['ind'], ss, tt, ssR, ttR, 20)
    np.testing.assert_allclose(R, f['R_hyp'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(t, f['t_hyp'], rtol=0, atol=1e-5)


def test_score_table_reproduces_fixture():
    """counts, winner and the winner's inliers are the fixture's exactly.  One (hypothesis, row) pair of the 1600 is undecided, (36, 9):
    float64 and the fixture's fp32 agree on it all the same, and it is not in the winner's row."""
    f, ss, tt, _, _ = _fixture()
    inl, und, thr = pose_ref.score_table(f['R_hyp'], f['t_hyp'], ss, tt, 20, 1 / 3, DELTA)
    assert np.argwhere(und).tolist() == [[36, 9]]
    num = inl.sum(1)
    assert np.array_equal(num, f['inlier_num'])
    assert int(np.argmax(num)) == int(f['best']) != 36
    assert np.array_equal(np.flatnonzero(inl[int(f['best'])]), f['inlier_ind'])
    np.testing.assert_allclose(thr, np.linalg.norm(ss.astype(np.float64), axis=1) * np.pi / 60, rtol=1e-15)


def test_score_table_skips_non_finite_rows():
    f, ss, tt, _, _ = _fixture()
    ss, tt = ss.copy(), tt.copy()
    ss[3], tt[7, 1] = np.nan, np.inf
    inl, und, _ = pose_ref.score_table(f['R_hyp'], f['t_hyp'], ss, tt, 20, 1 / 3, DELTA)
    assert not inl[:, [3, 7]].any() and not und[:, [3, 7]].any()
    keep = np.setdiff1d(np.arange(len(ss)), [3, 7])
    clean, _, _ = pose_ref.score_table(f['R_hyp'][keep], f['t_hyp'][keep], ss[keep], tt[keep], 20, 1 / 3, DELTA)
    assert np.array_equal(inl[np.ix_(keep, keep)], clean)


def test_post_refinement_reproduces_fixture():
    f, ss, tt, _, _ = _fixture()
    T, count, rounds, clear = pose_ref.post_refinement(f['init_pose'], ss, tt, 0.10, 20, DELTA)
    np.testing.assert_allclose(T, f['refined_pose'].reshape(4, 4), rtol=0, atol=2e-5)
    assert clear and rounds >= 1 and 0 < count <= len(ss)
    # rows with a non-finite coordinate are ignored
    ss2, tt2 = np.concatenate([ss, np.full((2, 3), np.nan, np.float32)]), np.concatenate([tt, np.full((2, 3), np.inf, np.float32)])
    T2, count2, rounds2, _ = pose_ref.post_refinement(f['init_pose'], ss2, tt2, 0.10, 20, DELTA)
    assert np.array_equal(T, T2) and (count, rounds) == (count2, rounds2)
    # iters = 0 and a start with no row under the threshold leave the pose alone
    far = np.array(f['init_pose'], np.float64).reshape(4, 4)
    far[:3, 3] += 10.0
    for T0, it in ((f['init_pose'], 0), (far, 20)):
        T3, count3, rounds3, _ = pose_ref.post_refinement(T0, ss, tt, 0.10, it, DELTA)
        assert np.array_equal(T3, np.asarray(T0, np.float64).reshape(4, 4)) and (count3, rounds3) == (0, 0)


def test_ransac_hypothesis_agrees_with_pipeline_ref():
    """on a 400-row planted set the best count over all hypotheses is pipeline_ref.ransac_kabsch's, and its winning index is a
    hypothesis that ransac_hypothesis scores with that count; a seed whose sums wrap 2^64 draws the same samples"""
    d = pose_ref.make_matches(4, 400, n_out=160, noise=0.01)
    corr = np.arange(400)
    for seed, nhyp in ((1, 512), ((1 << 64) - 301, 256)):
        T, (count, hstar) = pipeline_ref.ransac_kabsch(d['ss'], d['tt'], corr, nhyp, seed, 0.10, 0.8)
        hyp = [pose_ref.ransac_hypothesis(d['ss'], d['tt'], corr, seed, h, 0.10, 0.8, DELTA) for h in range(nhyp)]
        status = [h[0] for h in hyp]
        assert {pose_ref.EDGE, pose_ref.DIST, pose_ref.SCORED} == set(status)
        counts = np.array([h[2] for h in hyp])
        assert count == counts.max() and count >= 200
        assert hyp[hstar][0] == pose_ref.SCORED and hyp[hstar][2] == count
        assert hstar == min(h for h in range(nhyp) if counts[h] == count and hyp[h][3] == min(g[3] for g in hyp if g[2] == count))
        np.testing.assert_allclose(hyp[hstar][1], T, rtol=0, atol=1e-6)            # pipeline_ref returns float32
        assert np.abs(hyp[hstar][1] - d['T']).max() < 0.05
    assert pose_ref.ransac_hypothesis(d['ss'], d['tt'], corr[:2], 1, 0, 0.10, 0.8, DELTA)[0] == pose_ref.FEW


def test_sample_indices_are_distinct_and_cover_the_list():
    seen = set()
    for h in range(600):
        ids = pose_ref.sample_indices(7, h, 5)
        assert len(set(ids)) == 3 and all(0 <= i < 5 for i in ids)
        seen.add(ids)
    assert len(seen) == 60                                                      # every ordered triple of 5 is drawn
