"""Pose recovery (csrc/registration.hip) kernel by kernel against the float64 references of tests/pose_ref.py, at the sizes that cross
each strided loop of the file (64 in mask_compact, 256 in score_hypothesis and post_refine, 1024 in best_and_mask and ransac_pick), at
exact ties, on non-finite rows, and batched against pair by pair.

A count or a mask is compared exactly wherever the reference says that float64 and fp32 cannot disagree: pose_ref reports every
comparison that lies within DELTA = 1e-5 of its threshold as undecided, those are left out, and their share is bounded by an assertion
on the reference alone (it does not depend on the device).  Matrices are compared with the project's 1e-5 (hypotheses) and 2e-5 (poses);
util.assert_close prints the share of the tolerance that the worst element uses."""
from dataclasses import replace
from functools import lru_cache

import numpy as np
import pytest
import torch

import pair_chain
import pose_ref
from util import assert_close

pytestmark = pytest.mark.gpu
DELTA = 1e-5
MASK64 = (1 << 64) - 1
I4 = np.eye(4, dtype=np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _score(d, dev, azi_n=20, inlier_th=1 / 3):
    from buffer_amd import ops
    R, t, num, best, mask = ops.hypotheses_score(_t(d['ind'], dev), _t(d['ss'], dev), _t(d['tt'], dev), _t(d['ssR'], dev),
                                                 _t(d['ttR'], dev), azi_n, inlier_th)
    return R.cpu().numpy(), t.cpu().numpy(), num.cpu().numpy(), int(best.item()), mask.cpu().numpy()


def _rows(d, keep):
    return {k: (v[keep] if k in ('ind', 'ss', 'tt', 'ssR', 'ttR', 'bad') else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------ a. hypotheses and scoring
@pytest.mark.parametrize('inlier_th', [1 / 3, 2.0], ids=['th0.33', 'th2.0'])
@pytest.mark.parametrize('m', [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_hypotheses_and_scoring_vs_float64(dev, m, inlier_th):
    """m crosses the 256-row stride of score_hypothesis (once, four and eight times) and the 1024-row stride of best_and_mask."""
    d = pose_ref.make_matches(100 + m, m)
    R, t, num, best, mask = _score(d, dev, 20, inlier_th)
    Rr, tr = pose_ref.hypotheses(d['ind'], d['ss'], d['tt'], d['ssR'], d['ttR'], 20)
    assert_close(R, Rr, 0, 1e-5, f'R_hyp m={m}')
    assert_close(t, tr, 0, 1e-5, f't_hyp m={m}')
    # the scoring kernels read the device's own R and t: their decisions are referred to those, widened
    inl, und, _ = pose_ref.score_table(R, t, d['ss'], d['tt'], 20, inlier_th, DELTA)
    print(f'UNDECIDED scoring m={m} th={inlier_th:.2f}: {int(und.sum())} of {und.size} pairs, at most {int(und.sum(1).max())} per hypothesis')
    assert und.mean() <= 1e-4 and und.sum(1).max() <= 2                        # condition on the reference alone
    lo, hi = (inl & ~und).sum(1), (inl | und).sum(1)
    assert np.all((lo <= num) & (num <= hi)), f'counts outside the reference interval at hypotheses {np.flatnonzero((num < lo) | (num > hi))[:8]}'
    assert num.max() >= max(1, (m - d['bad'].sum()) // 4)                      # the planted motion is found: the counts are not trivial
    assert best == int(np.argmax(num))                                          # first maximum
    free = ~und[best]
    assert np.array_equal(mask[free] != 0, inl[best][free])
    assert set(np.unique(mask)) <= {0, 1}


def test_scoring_of_no_matches_is_a_no_op(dev):
    d = pose_ref.make_matches(1, 0)
    R, t, num, best, mask = _score(d, dev)
    assert R.shape == (0, 3, 3) and t.shape == (0, 3) and num.shape == (0,) and mask.shape == (0,) and best == 0


# ------------------------------------------------------------------------------------------ b. first maximum at exact ties
@pytest.mark.parametrize('pair', [(5, 1029), (70, 1030)])
def test_best_is_the_first_of_two_tied_maxima(dev, pair):
    """Two bit-identical rows (same ind, ss, tt and rotation rows) are the only ones that yield the planted rotation: their counts tie
    exactly (integer counts do not depend on the order of summation) and are the maximum.  (5, 1029) meet in one thread of best_and_mask
    on its two trips, (70, 1030) in different wavefronts."""
    m, (i, j) = 1100, pair
    d = pose_ref.make_matches(7, m, rot_share=0.0)
    g = int(np.flatnonzero(~d['bad'])[0])                                      # a good row lends its point pair
    ang = float(d['ind'][g]) * 2 * np.pi / 20 + 1e-6
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    win = (d['T'][:3, :3] @ d['ssR'][g].astype(np.float64) @ Rz.T).astype(np.float32)
    for k in ('ind', 'ss', 'tt', 'ssR'):
        d[k][i] = d[k][j] = d[k][g]
    d['ttR'][i] = d['ttR'][j] = win
    R, t, num, best, mask = _score(d, dev)
    assert np.array_equal(R[i], R[j]) and np.array_equal(t[i], t[j])
    assert num[i] == num[j] == num.max() and num[i] >= 100
    assert (num == num.max()).sum() == 2
    assert best == min(i, j)
    inl, und, _ = pose_ref.score_table(R, t, d['ss'], d['tt'], 20, 1 / 3, DELTA)
    free = ~und[best]
    assert np.array_equal(mask[free] != 0, inl[best][free])


def test_best_is_zero_when_every_count_is_zero(dev):
    """A row always fits its own hypothesis (t_h = tt_h - R_h ss_h), so moving tt away cannot empty the counts; a threshold of zero
    does: diff < 0 holds for no row.  All m = 1100 counts tie at 0 and the first one wins."""
    d = pose_ref.make_matches(8, 1100)
    d['tt'] += np.float32(3.0)
    R, t, num, best, mask = _score(d, dev, 20, 0.0)
    assert not num.any() and best == 0 and not mask.any()


# ------------------------------------------------------------------------------------------ c. non-finite rows
def test_non_finite_rows_count_nothing_and_change_nothing_else(dev):
    m = 300
    d = pose_ref.make_matches(9, m)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    c['ss'][3] = np.nan
    c['tt'][100, 1] = np.inf
    c['ss'][256, 2] = -np.inf
    c['tt'][299] = np.nan
    c['ss'][40, 0], c['tt'][40, 0] = np.inf, np.inf
    dirty = np.array([3, 40, 100, 256, 299])
    keep = np.setdiff1d(np.arange(m), dirty)
    _, _, num, best, mask = _score(c, dev)
    _, _, num_c, best_c, mask_c = _score(_rows(d, keep), dev)
    assert not num[dirty].any() and not mask[dirty].any()
    assert np.array_equal(num[keep], num_c)
    assert best == keep[best_c] and np.array_equal(mask[keep], mask_c)
    assert num_c.max() > 50


# ------------------------------------------------------------------------------------------ d. RANSAC, hypothesis by hypothesis
WRAP_SEED = (1 << 64) - 1501             # hypothesis 500 is seeded with 2^64 - 1: its second and third draw wrap inside the kernel
RANSAC_SETS = {                          # name: (rows, outliers, noise, seed of the run)
    'n400': (400, 160, 0.01, 1),
    'n64': (64, 20, 0.005, 2),
    'n7': (7, 2, 0.005, 3),
    'n3': (3, 0, 0.005, 4),
    'wrap': (64, 20, 0.005, WRAP_SEED),
}


@lru_cache(maxsize=None)
def _ransac_set(name):
    n, n_out, noise, seed = RANSAC_SETS[name]
    d = pose_ref.make_matches(20 + n, n, n_out=n_out, noise=noise)
    return d['ss'], d['tt'], seed


@lru_cache(maxsize=None)
def _ransac_ref(name, nhyp):
    """reference outcome of hypotheses 0 .. nhyp-1 of the set's run (computed once, shared, never changed)"""
    src, tgt, seed = _ransac_set(name)
    corr = np.arange(len(src))
    return tuple(pose_ref.ransac_hypothesis(src, tgt, corr, seed, h, 0.10, 0.8, DELTA) for h in range(nhyp))


def _ransac_single(src, tgt, corr, seeds):
    """hypothesis 0 of one run per seed with nhyp = 1 -> (T f32[k,4,4], info int32[k,2]), read back once"""
    from buffer_amd import ops
    out = [ops.ransac_kabsch(src, tgt, corr, nhyp=1, seed=int(s) & MASK64, max_dist=0.10, edge_similarity=0.8) for s in seeds]
    return torch.stack([o[0] for o in out]).cpu().numpy(), torch.stack([o[1] for o in out]).cpu().numpy()


@pytest.mark.parametrize('name', list(RANSAC_SETS))
def test_ransac_hypotheses_vs_float64(dev, name):
    """Hypothesis h of a run seeded s is hypothesis 0 of a run with nhyp = 1 seeded s + 3h (the kernel seeds its draws with
    splitmix64(seed + 3h + k)), so the public entry point shows the pose and the count of every single hypothesis."""
    src, tgt, seed = _ransac_set(name)
    nhyp = 1024
    ref = _ransac_ref(name, nhyp)
    und = np.array([r[4] for r in ref])
    scored = np.array([r[0] == pose_ref.SCORED and r[2] > 0 for r in ref])
    print(f'UNDECIDED ransac {name}: {int(und.sum())} of {nhyp} hypotheses; scored {int(scored.sum())}, '
          f'edge {sum(r[0] == pose_ref.EDGE for r in ref)}, dist {sum(r[0] == pose_ref.DIST for r in ref)}')
    assert und.mean() <= 0.01                                                    # condition on the reference alone
    assert scored.any() and (name == 'n3' or not scored.all())                   # both outcomes are exercised (n3: one triple, all or none)
    corr = torch.arange(len(src), dtype=torch.int32, device=dev)
    T, info = _ransac_single(_t(src, dev), _t(tgt, dev), corr, [seed + 3 * h for h in range(nhyp)])
    rej = ~und & ~scored
    assert np.array_equal(T[rej], np.broadcast_to(I4, T[rej].shape)) and np.all(info[rej] == [0, -1]), 'a rejected hypothesis returned a pose'
    ok = ~und & scored
    want_n = np.array([r[2] for r in ref])
    bad = np.flatnonzero(ok & ((info[:, 0] != want_n) | (info[:, 1] != 0)))
    assert bad.size == 0, f'hypotheses {bad[:8]}: device (count, index) {info[bad[:8]].tolist()} vs reference counts {want_n[bad[:8]].tolist()}'
    assert_close(T[ok], np.stack([r[1] for r in ref])[ok], 0, 2e-5, f'ransac T {name}')


# ------------------------------------------------------------------------------------------ e. RANSAC pick
def _pick(src, tgt, corr, nhyp, seed):
    from buffer_amd import ops
    T, info = ops.ransac_kabsch(src, tgt, corr, nhyp=nhyp, seed=seed, max_dist=0.10, edge_similarity=0.8)
    return T.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize('name,nhyp', [('n400', 4096), ('n400', 1), ('n400', 63), ('n400', 64), ('n400', 65), ('n400', 1025), ('wrap', 1025)])
def test_ransac_pick_returns_its_best_hypothesis(dev, name, nhyp):
    """nhyp crosses the wavefront granularity of the hypothesis launch (63, 64, 65) and the 1024 stride of ransac_pick (1025, 4096)."""
    src, tgt, seed = _ransac_set(name)
    ref = _ransac_ref(name, nhyp)
    s, g = _t(src, dev), _t(tgt, dev)
    corr = torch.arange(len(src), dtype=torch.int32, device=dev)
    T, info = _pick(s, g, corr, nhyp, seed)
    T2, info2 = _pick(s, g, corr, nhyp, seed)
    assert np.array_equal(T, T2) and np.array_equal(info, info2)                # reruns are bit-equal
    count, hs = int(info[0]), int(info[1])
    dec = np.array([not r[4] for r in ref])
    cnt = np.array([r[2] if r[0] == pose_ref.SCORED else 0 for r in ref])
    if hs == -1:                                                                # (nhyp = 1: the only hypothesis may be a rejected one)
        assert count == 0 and np.array_equal(T, I4) and not (dec & (cnt > 0)).any()
        return
    assert 0 <= hs < nhyp
    T1, info1 = _ransac_single(s, g, corr, [seed + 3 * hs])
    assert np.array_equal(T, T1[0]) and count == int(info1[0, 0])               # the pose and count of hypothesis h*, bit for bit
    assert dec[hs], f'winner {hs} is an undecided hypothesis: choose another seed'
    assert count == cnt[hs]
    assert cnt[dec].max() <= count, f'decided hypothesis {int(np.argmax(np.where(dec, cnt, -1)))} has a greater reference count'
    # among the decided hypotheses with the winning count none has a clearly smaller mean squared error: a pose within 2e-5 per entry
    # moves a point with |x| + |y| + |z| + 1 <= 3 by at most 6e-5 per axis, 1.1e-4 in norm, and a mean of squares d^2 by 2 rms 1.1e-4
    mse = np.array([r[3] for r in ref])
    rivals = np.flatnonzero(dec & (cnt == count))
    assert np.all(mse[rivals] >= mse[hs] - 2 * 2 * np.sqrt(mse[hs]) * 1.1e-4)   # (both sides of the comparison move)


def test_ransac_pick_takes_the_lowest_index_of_an_exact_tie(dev):
    """With three candidates every hypothesis draws one of the 6 orderings of the same triple, and equal orderings give bit-identical
    keys: the winner must be the first hypothesis that drew its ordering (restated sampler), whichever ordering wins."""
    src, tgt, _ = _ransac_set('n3')
    s, g = _t(src, dev), _t(tgt, dev)
    corr = torch.arange(3, dtype=torch.int32, device=dev)
    for seed, nhyp in ((4, 64), (11, 1025), (12, 2500)):
        T, info = _pick(s, g, corr, nhyp, seed)
        order = [pose_ref.sample_indices(seed, h, 3) for h in range(nhyp)]
        assert len(set(order)) == 6
        hs = int(info[1])
        assert int(info[0]) == 3 and hs == order.index(order[hs]), f'seed {seed}: picked {hs}, the first with its ordering is {order.index(order[hs])}'
        # every hypothesis with the winner's ordering returns the winner's pose
        same = [h for h in range(nhyp) if order[h] == order[hs]][:4] + [h for h in range(nhyp) if order[h] == order[hs]][-2:]
        T1, _ = _ransac_single(s, g, corr, [seed + 3 * h for h in same])
        assert all(np.array_equal(T, x) for x in T1)


@pytest.mark.parametrize('ncorr', [0, 1, 2])
def test_ransac_with_fewer_than_three_candidates_is_the_identity(dev, ncorr):
    src, tgt, _ = _ransac_set('n64')
    T, info = _pick(_t(src, dev), _t(tgt, dev), torch.arange(ncorr, dtype=torch.int32, device=dev), 65, 5)
    assert np.array_equal(T, I4) and info.tolist() == [0, -1]


# ------------------------------------------------------------------------------------------ f. masked form
def _masks(m):
    rng = np.random.default_rng(m)
    two = np.zeros(m, np.uint8)
    two[[m // 3, m - 1]] = 1
    late = np.zeros(m, np.uint8)
    late[64:] = rng.random(max(m - 64, 0)) < 0.7
    if m > 64:
        late[m - 1] = 1
    return {'ones': np.ones(m, np.uint8), 'zeros': np.zeros(m, np.uint8), 'two': two, 'past64': late,
            'random': (rng.random(m) < 0.6).astype(np.uint8) * np.uint8(3)}     # any non-zero byte is a set entry


@pytest.mark.parametrize('kind', ['ones', 'zeros', 'two', 'past64', 'random'])
@pytest.mark.parametrize('m', [63, 64, 65, 4097])
def test_masked_ransac_equals_ransac_on_the_listed_rows(dev, m, kind):
    """mask_compact (one wavefront, 64 entries per trip) + device-side count against the host-side index list: bit-equal pose and info.
    m = 63, 64, 65 cross one trip, 4097 takes 65."""
    from buffer_amd import ops
    d = pose_ref.make_matches(30 + m, m, n_out=m // 3, noise=0.005)
    mask = _masks(m)[kind]
    s, g = _t(d['ss'], dev), _t(d['tt'], dev)
    Tm, im = ops.ransac_kabsch_masked(s, g, _t(mask, dev), nhyp=256, seed=m, max_dist=0.10, edge_similarity=0.8)
    corr = _t(np.flatnonzero(mask).astype(np.int32), dev)
    Tc, ic = ops.ransac_kabsch(s, g, corr, nhyp=256, seed=m, max_dist=0.10, edge_similarity=0.8)
    assert torch.equal(Tm, Tc) and torch.equal(im, ic)
    if corr.shape[0] < 3:
        assert np.array_equal(Tm.cpu().numpy(), I4) and im.cpu().tolist() == [0, -1]
    elif kind in ('ones', 'random') or m == 4097:
        assert int(im[0]) >= 3 and int(im[1]) >= 0                              # a pose was found: the comparison is not of two identities


# ------------------------------------------------------------------------------------------ g. refinement
REFINE_THR = 0.10


def _refine_case(m, start, seed):
    """half the rows outliers at least 3 thr from their planted partner (m = 3 keeps all three rows: with two inliers the weighted
    Kabsch rotation is not unique, H has rank 1); start 1 = the planted pose, start 2 = that pose perturbed by 3 degrees and 5 cm"""
    d = pose_ref.make_matches(seed, m, n_out=0 if m == 3 else m // 2, noise=0.01, out_min=3 * REFINE_THR)
    T0 = d['T'] if start == 1 else pose_ref.small_motion(np.random.default_rng(seed + 1), 3.0, 0.05) @ d['T']
    return d['ss'], d['tt'], T0.astype(np.float32)


def _refine(dev, T0, src, tgt, thr, iters):
    from buffer_amd import ops
    T, info = ops.post_refine(_t(np.asarray(T0, np.float32), dev), _t(src, dev), _t(tgt, dev), thr, iters)
    return T.cpu().numpy(), info.cpu().tolist()


# seeds for which no distance of any round lies within DELTA of the threshold (pose_ref.post_refinement(...).clear), found on the CPU
# and, from the perturbed start, a first round that sees fewer inliers than the last
REFINE_SEEDS = {(255, 2): 47, (256, 2): 45, (257, 2): 41, (1000, 2): 45}       # every other case: 40


@pytest.mark.parametrize('start', [1, 2])
@pytest.mark.parametrize('m', [0, 1, 2, 3, 255, 256, 257, 1000])
def test_post_refine_vs_float64(dev, m, start):
    """m crosses the 256-row stride of post_refine and its cross-wave sums.  info = (inlier count of the last updating round, rounds)
    is exact; the pose is within the project's 2e-5.  With fewer than two inliers H is (numerically) zero and the rotation arbitrary:
    there the pose is held to what is determined, a proper rotation that carries the weighted centroid of the inliers onto its partner."""
    src, tgt, T0 = _refine_case(m, start, REFINE_SEEDS.get((m, start), 40))
    Tr, count, rounds, clear = pose_ref.post_refinement(T0, src, tgt, REFINE_THR, 20, DELTA)
    assert clear, 'choose another seed: a distance lies on the threshold'
    if m >= 255:                                                                # the planted start stops after one round, the perturbed one
        first = pose_ref.post_refinement(T0, src, tgt, REFINE_THR, 1, DELTA)[1]    # takes more and its count changes between them
        assert (rounds, count) == (1, m - m // 2) if start == 1 else (rounds >= 2 and first < count == m - m // 2), (first, count, rounds)
    T, info = _refine(dev, T0, src, tgt, REFINE_THR, 20)
    print(f'REFINE m={m} start={start}: count {count} rounds {rounds}')
    assert info == [count, rounds]
    assert np.array_equal(T[3], [0, 0, 0, 1])
    if count >= 3 or rounds == 0:
        assert_close(T, Tr, 0, 2e-5, f'refined pose m={m} start={start}')
    else:
        R = T[:3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and np.linalg.det(R) > 0.5
        x, b = src.astype(np.float64), tgt.astype(np.float64)
        inl = np.linalg.norm(x @ Tr[:3, :3].T + Tr[:3, 3] - b, axis=1) < REFINE_THR
        assert inl.sum() == count == 1
        assert np.abs(R @ x[inl][0] + T[:3, 3] - b[inl][0]).max() < 2e-5


def test_post_refine_zero_iterations_copies_the_pose(dev):
    src, tgt, T0 = _refine_case(257, 2, 41)
    T0 = T0.copy()
    T0[3] = [5, 6, 7, 8]                                                        # the last row is written, not copied
    T, info = _refine(dev, T0, src, tgt, REFINE_THR, 0)
    assert np.array_equal(T[:3], T0[:3]) and np.array_equal(T[3], [0, 0, 0, 1]) and info == [0, 0]


def test_post_refine_without_inliers_returns_its_start(dev):
    src, tgt, T0 = _refine_case(257, 1, 42)
    T0 = T0.copy()
    T0[:3, 3] += 10
    T, info = _refine(dev, T0, src, tgt, REFINE_THR, 20)
    assert np.array_equal(T, T0) and info == [0, 0]


def test_post_refine_ignores_non_finite_rows(dev):
    src, tgt, T0 = _refine_case(257, 2, 47)
    src, tgt = src.copy(), tgt.copy()
    src[5], tgt[64, 2], src[255, 0], tgt[256] = np.nan, np.nan, np.nan, np.nan
    tgt[130, 1] = np.inf
    Tr, count, rounds, clear = pose_ref.post_refinement(T0, src, tgt, REFINE_THR, 20, DELTA)
    assert clear and rounds >= 2
    T, info = _refine(dev, T0, src, tgt, REFINE_THR, 20)
    assert info == [count, rounds]
    assert_close(T, Tr, 0, 2e-5, 'refined pose beside non-finite rows')


def test_post_refine_at_outdoor_scale(dev):
    """coordinates up to 50 and thr = 1.2 as in the KITTI presets.  The fp32 rounding of a transformed point grows with its magnitude,
    so the bound is the project's 2e-5 times (largest |coordinate| / 1.2), and the undecided band scales the same way."""
    m, thr, scale = 1000, 1.2, 38.0
    d = pose_ref.make_matches(46, m, noise=0.1, out_min=3 * thr / scale, scale=scale)
    src, tgt = d['ss'], d['tt']
    big = float(max(np.abs(src).max(), np.abs(tgt).max()))
    assert 40 <= big <= 50
    T0 = pose_ref.small_motion(np.random.default_rng(47), 3.0, 0.8) @ d['T']
    Tr, count, rounds, clear = pose_ref.post_refinement(T0.astype(np.float32), src, tgt, thr, 20, DELTA * big / 1.15)
    assert clear and rounds >= 2 and count == m // 2
    T, info = _refine(dev, T0, src, tgt, thr, 20)
    assert info == [count, rounds]
    assert_close(T, Tr, 0, 2e-5 * big / 1.2, 'refined pose at outdoor scale')


# ------------------------------------------------------------------------------------------ h. batched == pair by pair
SEG_CYCLE = (0, 1, 2, 3, 4, 40, 257, 0, 1025, 5)


@lru_cache(maxsize=None)
def _pair(m, k):
    """matches of one pair; k varies the data between pairs of equal length"""
    d = pose_ref.make_matches(1000 + 7 * k + m, m, n_out=m // 3)
    return d['ind'], d['ss'], d['tt'], d['ssR'], d['ttR']


def _cfgs():
    from buffer_amd.config import KITTI, THREEDMATCH
    return {'refine': replace(THREEDMATCH, ransac_hypotheses=512), 'kitti': replace(KITTI, ransac_hypotheses=512)}


def _chain(dev, p, cfg, seed):
    """the chain of single-pair calls (tests/pair_chain.py)"""
    return pair_chain.recover_pose(*(_t(a, dev) for a in p), cfg, seed)


def _batched(dev, pairs, cfg, seeds):
    from buffer_amd import ops
    cat = [np.concatenate([p[i] for p in pairs]) if pairs else np.zeros((0,), np.float32) for i in range(5)]
    return ops.recover_poses_batched(*(_t(a, dev) for a in cat), [len(p[0]) for p in pairs], seeds, cfg)


@lru_cache(maxsize=None)
def _chain_cached(dev, m, k, name, seed):
    return _chain(dev, _pair(m, k), _cfgs()[name], seed).cpu().numpy()


def _check_batch(dev, lens, name, seeds=None, ks=None):
    cfg = _cfgs()[name]
    nb = len(lens)
    ks = [p // len(SEG_CYCLE) % 3 for p in range(nb)] if ks is None else ks    # three data sets per length: the per-pair side stays short
    seeds = [1000 + 17 * p for p in range(nb)] if seeds is None else seeds
    pairs = [_pair(m, k) for m, k in zip(lens, ks)]
    got = _batched(dev, pairs, cfg, seeds).cpu().numpy()
    assert got.shape == (nb, 4, 4)
    moved = 0
    for p, m in enumerate(lens):
        if m < 3:
            assert np.array_equal(got[p], I4), f'pair {p} of {m} rows is not the identity'
            continue
        want = _chain_cached(dev, m, ks[p], name, seeds[p])
        assert np.array_equal(got[p], want), f'pair {p} ({m} rows, seed {seeds[p]}) differs from the single-pair calls by {np.abs(got[p] - want).max()}'
        moved += not np.array_equal(want, I4)
    return got, moved


@pytest.mark.parametrize('name', ['refine', 'kitti'])
@pytest.mark.parametrize('nb', [1, 3, 65, 130])
def test_batched_recovery_equals_the_single_pair_calls(dev, nb, name):
    """nb = 65 crosses RB_MAXB = 64 pairs per RANSAC launch; 130 makes three RANSAC chunks and a second launch of the offsets upload
    (more than 127 pairs).  Segments of 0-3 rows sit beside long ones.  'kitti' is the refine_iters = 0 path, where the last kernel
    reads and writes the same buffer."""
    lens = [SEG_CYCLE[(p + (3 if nb <= 3 else 0)) % len(SEG_CYCLE)] for p in range(nb)]       # nb = 1: one pair of 3 rows; nb = 3: 3, 4, 40
    got, moved = _check_batch(dev, lens, name)
    if nb >= 3:
        assert moved >= sum(m >= 40 for m in lens)                              # the long pairs recover a pose: not identities compared


@pytest.mark.parametrize('name', ['refine', 'kitti'])
def test_batched_recovery_of_empty_and_one_sided_batches(dev, name):
    got, _ = _check_batch(dev, [0, 0, 0, 0], name)                               # M = 0
    assert np.array_equal(got, np.broadcast_to(I4, got.shape))
    _, moved = _check_batch(dev, [257, 0, 0, 0, 0], name)
    assert moved == 1
    _, moved = _check_batch(dev, [0, 0, 2, 0, 257], name)
    assert moved == 1


@pytest.mark.parametrize('name', ['refine', 'kitti'])
def test_batched_recovery_reversed_gives_the_poses_reversed(dev, name):
    lens = [SEG_CYCLE[p % len(SEG_CYCLE)] for p in range(70)]
    ks = [p // len(SEG_CYCLE) % 3 for p in range(70)]
    seeds = [1000 + 17 * p for p in range(70)]
    fwd, _ = _check_batch(dev, lens, name, seeds, ks)
    rev, _ = _check_batch(dev, lens[::-1], name, seeds[::-1], ks[::-1])
    assert np.array_equal(rev, fwd[::-1])
