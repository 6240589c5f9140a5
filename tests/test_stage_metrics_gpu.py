"""Per-stage ground-truth metrics on the device (buf_match_metrics, BufferPipeline.register_batch(metrics_gt=), --stage-metrics).

The reference of every count is the numpy restatement below of the arithmetic include/buffer_hip.h defines; it does not call into
buffer_amd.  Counts are compared for equality and out_nn_d2 bit for bit: the arithmetic is defined so that no tolerance is needed."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest

COLS = ('rep_src', 'rep_tgt', 'nn_inl', 'mutual', 'mutual_inl', 'cons', 'cons_true')
F32 = np.float32


# ------------------------------------------------------------------------------------------- the numpy restatement
def ref_apply(T, pts):
    """p = T s in fp64 without FMA, ((r0*x + r1*y) + r2*z) + t, rounded to fp32.  T f64[4,4], pts f32[n,3] -> f32[n,3]"""
    T = np.asarray(T, np.float64)
    x, y, z = (np.asarray(pts, F32)[:, i].astype(np.float64) for i in range(3))
    with np.errstate(all='ignore'):
        return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]) for r in range(3)], axis=1).astype(F32)


def ref_inverse(T):
    """[R^T, -R^T t] in fp64: tinv_i = -((R0i*t0 + R1i*t1) + R2i*t2)"""
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return out


def ref_d2(p, q):
    """(dx*dx + dy*dy) + dz*dz in fp32 (broadcasting over leading axes)"""
    with np.errstate(all='ignore'):
        d = np.asarray(p, F32) - np.asarray(q, F32)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def ref_nearest(p, refs):
    """running minimum over ascending rows with a strict <: (d2 f32[n] (+inf where nothing compares below it), row int[n] or -1).
    A NaN d2 never wins; among equal d2 the lowest row stays."""
    if len(refs) == 0:
        return np.full(len(p), np.inf, F32), np.full(len(p), -1)
    d = ref_d2(p[:, None, :], refs[None, :, :])
    d = np.where(np.isnan(d), F32(np.inf), d)
    row = d.argmin(axis=1)                                     # first occurrence = lowest row
    best = d[np.arange(len(p)), row]
    return best.astype(F32), np.where(np.isinf(best), -1, row)


def ref_pair(kp_s, kp_t, s_nn, t_nn, T_gt, T_est, tau_kp, tau_match, dist_th):
    """-> (counts int[7], nn_d2 of the source rows f32[P], nn_d2 of the target rows f32[P])"""
    P = len(kp_s)
    kp2, match2, cons2 = (F32(t) * F32(t) for t in (tau_kp, tau_match, dist_th))
    p = ref_apply(T_gt, kp_s)
    d_src, _ = ref_nearest(p, kp_t)
    d_tgt, _ = ref_nearest(ref_apply(ref_inverse(T_gt), kp_t), kp_s)
    s_nn, t_nn = np.asarray(s_nn, np.int64), np.asarray(t_nn, np.int64)
    valid = (s_nn >= 0) & (s_nn < P)
    t = np.where(valid, s_nn, 0)
    q = kp_t[t] if P else kp_t
    nn_inl = valid & (ref_d2(p, q) < match2)
    mutual = valid & (t_nn[t] == np.arange(P)) if P else valid
    cons = mutual & (ref_d2(ref_apply(np.asarray(T_est, F32).astype(np.float64), kp_s), q) < cons2)
    counts = [(d_src < kp2).sum(), (d_tgt < kp2).sum(), nn_inl.sum(), mutual.sum(), (mutual & nn_inl).sum(), cons.sum(),
              (cons & nn_inl).sum()]
    return np.array(counts, np.int64), d_src, d_tgt


def ref_batch(kp, s_nn, t_nn, T_gt, T_est, tau_kp, tau_match, dist_th):
    B, P = s_nn.shape
    counts, d2 = [], []
    for b in range(B):
        c, ds, dt = ref_pair(kp[2 * b * P:(2 * b + 1) * P], kp[(2 * b + 1) * P:(2 * b + 2) * P], s_nn[b], t_nn[b], T_gt[b], T_est[b],
                             tau_kp, tau_match, dist_th)
        counts.append(c)
        d2 += [ds, dt]
    return np.stack(counts), (np.concatenate(d2) if d2 else np.zeros(0, F32))


# ------------------------------------------------------------------------------------------- random cases
def random_rigid(rng, max_angle=np.pi, max_t=0.5):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rng.uniform(-max_t, max_t, 3)
    return T


TAU_KP, TAU_MATCH, DIST_TH = 0.03125, 0.0625, 0.125          # dyadic: tau * tau is exact in fp32, and so is p - tau below


def _plant(kp_t, j, p, tau, axis):
    """target row j at EXACTLY the distance tau from the fp32 point p along one axis (d2 == tau*tau, so NOT within tau).  The
    offset goes to the side (and, failing that, the axis) where p -/+ tau is an fp32 number, so that the difference is tau itself."""
    for ax in (axis, (axis + 1) % 3, (axis + 2) % 3):
        for sign in (1, -1):
            q = p.copy()
            q[ax] = F32(p[ax] - F32(sign * tau))
            if abs(F32(p[ax] - q[ax])) == F32(tau):
                kp_t[j] = q
                assert ref_d2(p, q) == F32(tau) * F32(tau)
                return
    raise AssertionError('no exact offset found for the planted point')


def make_case(B, P, seed):
    """random keypoints in [-1,1]^3, random 1-NN rows (a third of them made mutual), random rigid T_gt and a T_est near it; where
    the cloud is large enough: keypoints planted exactly at each threshold distance, duplicate target keypoints, a NaN row and an
    inf row, and an out-of-range match index."""
    rng = np.random.default_rng(seed)
    kp = rng.uniform(-1, 1, (2 * B * P, 3)).astype(F32)
    s_nn = rng.integers(0, max(P, 1), (B, P)).astype(np.int32)
    t_nn = rng.integers(0, max(P, 1), (B, P)).astype(np.int32)
    T_gt = np.stack([random_rigid(rng) for _ in range(B)]) if B else np.zeros((0, 4, 4))
    T_est = np.stack([(random_rigid(rng, 0.02, 0.02) @ T_gt[b]).astype(F32) for b in range(B)]) if B else np.zeros((0, 4, 4), F32)
    planted = 0
    for b in range(B):
        src, tgt = kp[2 * b * P:(2 * b + 1) * P], kp[(2 * b + 1) * P:(2 * b + 2) * P]
        # targets near the transformed sources, so that every count is far from 0 and from P
        near = rng.permutation(P)[:P // 2]
        tgt[near] = ref_apply(T_gt[b], src[near]) + rng.normal(0, 0.03, (len(near), 3)).astype(F32)
        s_nn[b, near[:len(near) // 2]] = near[:len(near) // 2]
        mut = rng.permutation(P)[:P // 3]
        t_nn[b, s_nn[b, mut]] = mut
        if P >= 64:
            p_gt, p_est = ref_apply(T_gt[b], src), ref_apply(T_est[b].astype(np.float64), src)
            _plant(tgt, 1, p_gt[0], TAU_KP, 0)                  # repeatability: source 0 sees target 1 exactly at tau_kp
            _plant(tgt, 3, p_gt[2], TAU_MATCH, 1)               # match inlier distance, a mutual match
            s_nn[b, 2], t_nn[b, 3] = 3, 2
            _plant(tgt, 5, p_est[4], DIST_TH, 2)                # consensus distance under T_est, a mutual match
            s_nn[b, 4], t_nn[b, 5] = 5, 4
            tgt[7] = tgt[6]                                     # duplicate target keypoints: a tie in every distance
            tgt[8] = tgt[6]
            src[9] = (np.nan, 0.5, 0.5)                         # non-finite points are within nothing
            tgt[10] = (0.25, np.inf, 0.0)
            s_nn[b, 11] = 10                                    # a match onto the inf row
            s_nn[b, 12], s_nn[b, 13] = -1, P                    # indices outside the cloud match nothing
            planted += 1
    return kp, s_nn, t_nn, T_gt, T_est, planted


def test_reference_sees_the_planted_points():
    """(no device) the planted points sit exactly ON the thresholds in the reference's own arithmetic, and count as outside"""
    kp, s_nn, t_nn, T_gt, T_est, planted = make_case(1, 257, 7)
    assert planted == 1
    P = 257
    src, tgt = kp[:P], kp[P:]
    p = ref_apply(T_gt[0], src)
    assert ref_d2(p[0], tgt[1]) == F32(TAU_KP) ** 2 and ref_d2(p[2], tgt[3]) == F32(TAU_MATCH) ** 2
    assert ref_d2(ref_apply(T_est[0].astype(np.float64), src)[4], tgt[5]) == F32(DIST_TH) ** 2
    c, d_src, d_tgt = ref_pair(src, tgt, s_nn[0], t_nn[0], T_gt[0], T_est[0], TAU_KP, TAU_MATCH, DIST_TH)
    assert np.isinf(d_src[9]) and np.isfinite(np.delete(d_src, 9)).all()       # the NaN source row has no nearest keypoint
    assert np.isinf(d_tgt[10])
    # moving a threshold up by one ulp takes the planted point in: it was exactly on the edge
    up = lambda t: float(np.nextafter(F32(t), F32(1)))
    c_kp = ref_pair(src, tgt, s_nn[0], t_nn[0], T_gt[0], T_est[0], up(TAU_KP), TAU_MATCH, DIST_TH)[0]
    c_m = ref_pair(src, tgt, s_nn[0], t_nn[0], T_gt[0], T_est[0], TAU_KP, up(TAU_MATCH), DIST_TH)[0]
    c_c = ref_pair(src, tgt, s_nn[0], t_nn[0], T_gt[0], T_est[0], TAU_KP, TAU_MATCH, up(DIST_TH))[0]
    if d_src[0] == F32(TAU_KP) ** 2:                                            # (unless a random target came nearer still)
        assert c_kp[0] >= c[0] + 1
    assert c_m[2] >= c[2] + 1 and c_m[4] >= c[4] + 1 and c_c[5] >= c[5] + 1
    assert 0 < c[3] < P and 0 < c[0] < P and 0 < c[2] < P and 0 < c[5] <= c[3]
    _, row = ref_nearest(np.stack([tgt[6]]), tgt)
    assert row[0] == 6                                                          # tie between rows 6, 7, 8 -> the lowest


# ------------------------------------------------------------------------------------------- 1. exact against numpy
def _device_metrics(dev, kp, s_nn, t_nn, T_gt, T_est, want_d2=True):
    import torch
    from buffer_amd import ops
    out = ops.match_metrics(torch.from_numpy(kp).to(dev), torch.from_numpy(s_nn).to(dev), torch.from_numpy(t_nn).to(dev),
                            torch.from_numpy(T_gt).to(dev), torch.from_numpy(T_est).to(dev), TAU_KP, TAU_MATCH, DIST_TH, want_d2=want_d2)
    if want_d2:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1500])
def test_match_metrics_equal_numpy(dev, B, P):
    kp, s_nn, t_nn, T_gt, T_est, planted = make_case(B, P, 1000 * B + P)
    assert planted == (B if P >= 64 else 0)
    want_c, want_d2 = ref_batch(kp, s_nn, t_nn, T_gt, T_est, TAU_KP, TAU_MATCH, DIST_TH)
    got_c, got_d2 = _device_metrics(dev, kp, s_nn, t_nn, T_gt, T_est)
    print(f'STAGE_METRICS B={B} P={P} counts device {got_c.tolist()} numpy {want_c.tolist()}')
    assert got_c.dtype == np.int32 and got_c.shape == (B, 7)
    assert np.array_equal(got_c, want_c)
    assert got_d2.dtype == F32 and np.array_equal(got_d2.view(np.uint32), want_d2.view(np.uint32))
    assert np.array_equal(_device_metrics(dev, kp, s_nn, t_nn, T_gt, T_est, want_d2=False), want_c)     # out_nn_d2 = NULL


@pytest.mark.gpu
def test_match_metrics_empty(dev):
    import torch
    from buffer_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    c, d2 = ops.match_metrics(z(0, 3), z(0, 5, dt=torch.int32), z(0, 5, dt=torch.int32), z(0, 4, 4, dt=torch.float64), z(0, 4, 4), 0.1, 0.1,
                              0.1, want_d2=True)
    assert tuple(c.shape) == (0, 7) and tuple(d2.shape) == (0,)
    c = ops.match_metrics(z(0, 3), z(2, 0, dt=torch.int32), z(2, 0, dt=torch.int32), z(2, 4, 4, dt=torch.float64), z(2, 4, 4), 0.1, 0.1, 0.1)
    assert tuple(c.shape) == (2, 7)                              # P = 0: the entry point touches nothing (rows undefined)


# ------------------------------------------------------------------------------------------- 2. batch independence
@pytest.mark.gpu
def test_match_metrics_batch_independent_and_deterministic(dev):
    P = 700
    kp, s_nn, t_nn, T_gt, T_est, _ = make_case(4, P, 99)
    full_c, full_d2 = _device_metrics(dev, kp, s_nn, t_nn, T_gt, T_est)
    again_c, again_d2 = _device_metrics(dev, kp, s_nn, t_nn, T_gt, T_est)
    assert np.array_equal(full_c, again_c) and np.array_equal(full_d2.view(np.uint32), again_d2.view(np.uint32))
    for b in range(4):
        rows = slice(2 * b * P, (2 * b + 2) * P)
        alone_c, alone_d2 = _device_metrics(dev, kp[rows].copy(), s_nn[b:b + 1], t_nn[b:b + 1], T_gt[b:b + 1], T_est[b:b + 1])
        assert np.array_equal(alone_c[0], full_c[b]), b
        assert np.array_equal(alone_d2.view(np.uint32), full_d2[rows].view(np.uint32)), b
    # pair 0 at every position of a batch of 4 (swapped with the pair that sat there)
    for pos in range(4):
        order = list(range(4))
        order[pos], order[0] = 0, pos
        kp2 = np.concatenate([kp[2 * b * P:(2 * b + 2) * P] for b in order])
        c2, d22 = _device_metrics(dev, kp2, s_nn[order], t_nn[order], T_gt[order], T_est[order])
        assert np.array_equal(c2[pos], full_c[0]), pos
        assert np.array_equal(d22[2 * pos * P:(2 * pos + 2) * P].view(np.uint32), full_d2[:2 * P].view(np.uint32)), pos


# ------------------------------------------------------------------------------------------- 3. pipeline
def _check_invariants(counts, P):
    c = {k: counts[:, i] for i, k in enumerate(COLS)}
    assert (0 <= c['mutual_inl']).all() and (c['mutual_inl'] <= c['mutual']).all() and (c['mutual'] <= P).all()
    assert (0 <= c['cons_true']).all() and (c['cons_true'] <= c['cons']).all() and (c['cons'] <= c['mutual']).all()
    assert (0 <= c['rep_src']).all() and (c['rep_src'] <= P).all() and (0 <= c['rep_tgt']).all() and (c['rep_tgt'] <= P).all()
    assert (0 <= c['nn_inl']).all() and (c['nn_inl'] <= P).all()


@pytest.fixture(scope="module")
def pairs():
    from buffer_amd import synth
    return [synth.make_pair(11, n_raw=40_000, size=(1.0, 1.0, 0.9), n_boxes=3),
            synth.make_pair(12, n_raw=40_000, size=(1.0, 1.0, 0.9), n_boxes=3)]


def _ref_from_detail(pipe, inp, seed, gt, pose, d):
    """the numpy reference fed from register(detail=True): all columns through ops.knn on the detail descriptors, and the mutual
    column and its derivatives once more from s_mids / t_mids alone"""
    from buffer_amd import ops
    P, th = pipe.cfg.num_keypts, pipe.cfg.dist_th
    kp_s, kp_t = (k.cpu().numpy() for k in d['kpts'])
    _, s_idx = ops.knn(d['desc'][1]['desc'][None], d['desc'][0]['desc'][None], 1)
    _, t_idx = ops.knn(d['desc'][0]['desc'][None], d['desc'][1]['desc'][None], 1)
    s_nn, t_nn = s_idx[0, :, 0].cpu().numpy(), t_idx[0, :, 0].cpu().numpy()
    T_est = pose.cpu().numpy()
    full = ref_pair(kp_s, kp_t, s_nn, t_nn, gt, T_est, th, th, th)[0]
    s_only, t_only = np.full(P, -1), np.full(P, -1)
    s_mids, t_mids = d['s_mids'].cpu().numpy(), d['t_mids'].cpu().numpy()
    s_only[s_mids], t_only[t_mids] = t_mids, s_mids
    mids = ref_pair(kp_s, kp_t, s_only, t_only, gt, T_est, th, th, th)[0]
    assert mids[3] == len(s_mids) and np.array_equal(mids[3:], full[3:])
    return full


@pytest.mark.gpu
def test_pipeline_metrics_rows_and_identical_poses(pairs, dev):
    import torch
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.pipeline import BufferPipeline
    pipe = BufferPipeline(replace(THREEDMATCH, num_keypts=300), dev)
    pipe.calibrate([pairs[0]])
    inps = [pipe.upload(pairs[0]), pipe.upload(pairs[1]), pipe.upload(pairs[0])]
    gts = [pairs[0]['relt_pose'], pairs[1]['relt_pose'], pairs[0]['relt_pose']]
    seeds = [0, 1, 2]
    plain = pipe.register_batch(inps, seeds=seeds)
    poses, counts = pipe.register_batch(inps, seeds=seeds, metrics_gt=gts)
    assert isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (3, 7)
    for a, b in zip(plain, poses):
        assert torch.equal(a, b)                                 # bit-identical poses with metrics on
    counts = counts.cpu().numpy()
    for b in range(3):
        pose, d = pipe.register(inps[b], seed=seeds[b], detail=True)
        assert torch.equal(pose, poses[b])
        want = _ref_from_detail(pipe, inps[b], seeds[b], gts[b], pose, d)
        print(f'STAGE_METRICS pipeline pair {b}: device {counts[b].tolist()} numpy {want.tolist()}')
        assert np.array_equal(counts[b], want), b
        # register()'s own row (the kernel at B = 1) is the batch's row
        p1, row = pipe.register(inps[b], seed=seeds[b], metrics_gt=gts[b])
        assert torch.equal(p1, poses[b]) and np.array_equal(row.cpu().numpy(), counts[b])
    _check_invariants(counts, 300)
    # the thresholds are keywords: a consensus distance of 1 km takes every mutual match in, tiny ones take nothing
    _, wide = pipe.register_batch(inps, seeds=seeds, metrics_gt=np.stack(gts), dist_th=1000.0, tau_kp=1e-6, tau_match=1e-6)
    wide = wide.cpu().numpy()
    assert np.array_equal(wide[:, 5], counts[:, 3]) and np.array_equal(wide[:, 3], counts[:, 3])
    assert (wide[:, [0, 1, 2, 4, 6]] == 0).all()
    with pytest.raises(ValueError):
        pipe.register_batch(inps, seeds=seeds, metrics_gt=gts[:2])


@pytest.mark.gpu
def test_register_batches_metrics_equal_batch_by_batch(pairs, dev):
    import torch
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.pipeline import BufferPipeline
    pipe = BufferPipeline(replace(THREEDMATCH, num_keypts=300), dev)
    pipe.calibrate([pairs[0]])
    a, b = pipe.upload(pairs[0]), pipe.upload(pairs[1])
    ga, gb = pairs[0]['relt_pose'], pairs[1]['relt_pose']
    batches, gts, seeds = [[a, b], [b], [b, a, a]], [[ga, gb], [gb], [gb, ga, ga]], [[0, 1], [2], [3, 4, 5]]
    want = [pipe.register_batch(x, seeds=s, metrics_gt=g) for x, s, g in zip(batches, seeds, gts)]
    plain = pipe.register_batches(batches, seeds=seeds)
    got = pipe.register_batches(batches, seeds=seeds, metrics_gt=[gts[0], (lambda: gts[1]), gts[2]])     # (a callable is fine too)
    assert len(got) == 3
    for (gp, gc), (wp, wc), pp in zip(got, want, plain):
        assert torch.equal(gc, wc) and len(gp) == len(wp) == len(pp)
        for x, y, z in zip(gp, wp, pp):
            assert torch.equal(x, y) and torch.equal(x, z)
    assert pipe.register_batches([], metrics_gt=[]) == []


# ------------------------------------------------------------------------------------------- 4. fallback rows
@pytest.mark.gpu
def test_starved_pair_gets_a_row_of_minus_one(pairs, dev):
    """the starved path of tests/test_pipeline_gpu.py (keypts_th raised above one pair's top score): the starved pair's row
    is -1 everywhere, the healthy pair's row is the one it gets alone, the poses are those of a call without metrics"""
    import torch
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.pipeline import BufferPipeline
    cfg = replace(THREEDMATCH, num_keypts=200)
    probe = BufferPipeline(cfg, dev)
    probe.calibrate([pairs[0]])
    tops = []
    for s in pairs:
        _, d = probe.register(probe.upload(s), seed=0, detail=True)
        n_src = int(probe.upload(s)['lengths'][0])
        sc = d['score'][:, 0]
        tops.append(min(float(sc[:n_src].max()), float(sc[n_src:].max())))
    lo, hi = sorted(tops)
    assert lo < hi, 'the two pairs peak at the same score: the fixture cannot force the starved path'
    starved = 0 if tops[0] == lo else 1
    healthy = 1 - starved
    # the threshold AT the starved pair's top score (the comparison is a strict >): its weaker cloud keeps no point, the other
    # pair keeps every point that scores higher, which is enough of them to be matched and evaluated
    pipe = BufferPipeline(replace(cfg, keypts_th=lo), dev, limits=probe.limits)
    inps = [pipe.upload(s) for s in pairs]
    gts = [s['relt_pose'] for s in pairs]
    plain = pipe.register_batch(inps, seeds=[3, 4])
    poses, counts = pipe.register_batch(inps, seeds=[3, 4], metrics_gt=gts)
    assert torch.equal(plain[0], poses[0]) and torch.equal(plain[1], poses[1])
    assert torch.equal(poses[starved], torch.eye(4, device=dev))
    counts = counts.cpu().numpy()
    print(f'STAGE_METRICS starved path: tops {tops} rows {counts.tolist()}')
    assert counts.dtype == np.int32 and (counts[starved] == -1).all()
    alone_pose, alone = pipe.register_batch([inps[healthy]], seeds=[[3, 4][healthy]], metrics_gt=[gts[healthy]])
    assert torch.equal(alone_pose[0], poses[healthy])
    assert np.array_equal(alone.cpu().numpy()[0], counts[healthy]) and (counts[healthy] >= 0).all()
    _check_invariants(counts[healthy:healthy + 1], 200)
    # the starved pair alone: register() answers with the identity and a row of -1
    p, row = pipe.register(inps[starved], seed=3, metrics_gt=gts[starved])
    assert torch.equal(p, torch.eye(4, device=dev)) and (row.cpu().numpy() == -1).all()
    # the same through register_batches
    (bp, bc), = pipe.register_batches([inps], seeds=[[3, 4]], metrics_gt=[gts])
    assert np.array_equal(bc.cpu().numpy(), counts) and torch.equal(bp[healthy], poses[healthy])


# ------------------------------------------------------------------------------------------- 5. drivers
def _tree(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def _main(mod, argv, capsys):
    poses = mod.main(argv)
    out = json.loads([ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith('{')][-1])
    return poses, out


def _check_driver(mod, base_argv, n_pairs, scenes, P, tmp_path, capsys, plain_keys_gone=('pairs_per_sec',)):
    from buffer_amd import evaluate
    logs0, logs1 = str(tmp_path / 'logs_plain'), str(tmp_path / 'logs_stage')
    p0, out0 = _main(mod, base_argv + ['--log-root', logs0], capsys)
    lim = ','.join(map(str, out0['limits']))
    p1, out1 = _main(mod, base_argv + ['--log-root', logs1, '--limits', lim, '--stage-metrics'], capsys)
    assert np.array_equal(p0, p1)                                                 # the poses do not move
    assert 'stage' not in out0 and set(out1) == set(out0) | {'stage'}
    for k in out0:
        if k not in plain_keys_gone:
            assert json.dumps(out0[k]) == json.dumps(out1[k]), k
    t0, t1 = _tree(logs0), _tree(logs1)
    assert 'stage_metrics.json' not in t0 and set(t1) == set(t0) | {'stage_metrics.json'}
    for k in t0:
        assert t0[k] == t1[k], f'{k} differs with --stage-metrics'               # logs byte-identical
    rec = json.loads(t1['stage_metrics.json'])
    assert rec['columns'] == list(COLS) and rec['num_keypts'] == P and len(rec['pairs']) == n_pairs
    counts = np.array([r['counts'] for r in rec['pairs']])
    ev = counts[(counts >= 0).all(1)]
    _check_invariants(ev, P)
    assert ((counts >= 0).all(1) | (counts == -1).all(1)).all()
    stage = out1['stage']
    assert rec['summary'] == stage
    print('STAGE_METRICS driver', mod.__name__, json.dumps(stage))
    want = evaluate.stage_summary(counts, P)
    for k, v in want.items():
        assert stage[k] == v, k
    assert list(stage['per_scene']) == list(scenes)
    n = sum(v['pairs'] for v in stage['per_scene'].values())
    assert n == stage['pairs'] and n + stage['not_evaluated'] == n_pairs
    for k in ('repeatability', 'inlier_ratio', 'fmr', 'mutual_inlier_ratio', 'consensus_precision'):
        if n:
            assert abs(sum(v[k] * v['pairs'] for v in stage['per_scene'].values()) / n - stage[k]) < 1e-12, k
    return rec, p1


@pytest.mark.gpu
def test_threedmatch_driver_stage_metrics(tmp_path, dev, capsys):
    from buffer_amd import threedmatch as tdm
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    scenes = tdm.SCENES
    _mini_dataset(root, scenes, seed=5)
    rec, _ = _check_driver(tdm, ['--root', root, '--log-name', 'cli.log', '--batch', '8'], 24, scenes, 1500, tmp_path, capsys)
    ds = tdm.ThreeDMatchTestSet(root)
    assert [r['id'] for r in rec['pairs']] == [f'{s} {t}' for s, t in ds.files]  # one row per pair in data-set order


@pytest.mark.gpu
def test_eth_driver_stage_metrics(tmp_path, dev, capsys):
    from buffer_amd import eth, synth
    root = str(tmp_path / 'eth')
    scenes = ['gazebo_summer', 'wood_autmn']
    synth.make_eth_root(root, scenes=scenes, stations=3, seed=11, non_finite_rows=3)
    rec, _ = _check_driver(eth, ['--root', root, '--scenes'] + scenes + ['--batch', '4'], 6, scenes, 1500, tmp_path, capsys)
    ds = eth.ETHTestSet(root, scenes)
    assert [r['id'] for r in rec['pairs']] == [f'{s} {t}' for s, t in ds.files]
