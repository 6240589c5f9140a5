"""Batched matching above the kernel, on the self-registration pairs of tests/test_fpfh_register_gpu.py: FpfhRegistration, which now
takes the matches of a whole batch from ONE fpfh.match_batch call, gives for each of its four estimators the poses, bit for bit, that
the same estimator calls give on matches made pair by pair with fpfh.match (the parent's path: two ops.knn calls per pair);
match_ratio thins the matches and keeps the poses inside the DGR thresholds; the driver's --match-ratio; the open3d stand-in's
correspondences_from_features."""
import json

import numpy as np
import pytest
import torch

from test_fpfh_register_gpu import _pair, _upload

pytestmark = pytest.mark.gpu
RATIO = 0.8


@pytest.fixture(scope='module')
def pairs():
    return [_pair(11, 0.7), _pair(12, 2.1)]


@pytest.fixture(scope='module')
def described(dev, pairs):
    """what register_batch sees of the two pairs: (inps, pts, lens, off, F) and the pair-by-pair fpfh.match lists"""
    from buffer_amd import fpfh
    from buffer_amd.config import THREEDMATCH
    reg = fpfh.FpfhRegistration(THREEDMATCH, dev)
    inps = [_upload(p, dev) for p, _ in pairs]
    pts = torch.cat([i['points'] for i in inps]).float().contiguous()
    nrm = torch.cat([i['features'][:, :3] for i in inps]).float().contiguous()
    lens = np.concatenate([np.asarray(i['lengths'], np.int32).reshape(2) for i in inps])
    F = fpfh.compute_fpfh(pts, nrm, reg.radius, reg.max_nn, lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    corrs = [fpfh.match(F[off[2 * b]:off[2 * b + 1]], F[off[2 * b + 1]:off[2 * b + 2]], True) for b in range(len(inps))]
    return dict(inps=inps, pts=pts, lens=lens, off=off, F=F, corrs=corrs)


def _poses_from(reg, d, corrs, seeds, estimator):
    """the estimator calls of FpfhRegistration on the given per-pair match lists"""
    from buffer_amd import clique, fgr, fpfh, ops, sc2
    pts, lens, off, B = d['pts'], d['lens'], d['off'], len(corrs)
    if estimator == 'ransac':
        return [fpfh.ransac_on_matches(pts[off[2 * b]:off[2 * b + 1]], pts[off[2 * b + 1]:off[2 * b + 2]], corrs[b],
                                       reg.cfg.ransac_hypotheses, seeds[b], reg.max_dist, reg.edge_similarity) for b in range(B)]
    src = torch.cat([pts[off[2 * b]:off[2 * b + 1]] for b in range(B)])
    tgt = torch.cat([pts[off[2 * b + 1]:off[2 * b + 2]] for b in range(B)])
    corr, cl = torch.cat(corrs), [int(c.shape[0]) for c in corrs]
    if estimator == 'fgr':
        res = fgr.fast_global_registration(src, lens[0::2], tgt, lens[1::2], corr, cl, seeds=[int(s) & ops._MASK64 for s in seeds],
                                           maximum_correspondence_distance=reg.max_dist, delta_absolute=True)
    elif estimator == 'sc2':
        res = sc2.sc2_registration(src, lens[0::2], tgt, lens[1::2], corr, cl, d_thr=reg.max_dist, inlier_thr=reg.max_dist, nms_radius=0.0)
    else:
        res = clique.clique_registration(src, lens[0::2], tgt, lens[1::2], corr, cl, d_thr=reg.max_dist, tim_thr=reg.max_dist,
                                         t_thr=reg.max_dist / 2, inlier_thr=reg.max_dist)
    return list(res['poses'].float().unbind(0))


def test_match_batch_gives_the_pair_by_pair_lists(dev, described):
    from buffer_amd import fpfh
    d = described
    corr, cl = fpfh.match_batch(d['F'], d['lens'])
    assert cl.tolist() == [int(c.shape[0]) for c in d['corrs']] and min(cl) >= 3 and torch.equal(corr, torch.cat(d['corrs']))
    # the ratio test thins the lists: sub-lists of the unfiltered ones, in order (how many it drops on a scene matched onto its own
    # copy is printed, not asserted: tests/test_match_gpu.py has the cases on which it must drop some)
    thin, tl = fpfh.match_batch(d['F'], d['lens'], True, RATIO)
    co, to = np.concatenate([[0], np.cumsum(cl)]), np.concatenate([[0], np.cumsum(tl)])
    for b in range(2):
        full = [tuple(r) for r in corr[co[b]:co[b + 1]].cpu().numpy()]
        kept = [tuple(r) for r in thin[to[b]:to[b + 1]].cpu().numpy()]
        print(f'pair {b}: {len(full)} mutual matches, {len(kept)} after the ratio test at {RATIO}')
        assert set(kept) <= set(full) and kept == sorted(kept) and 3 <= len(kept) <= len(full)


@pytest.mark.parametrize('estimator', ['ransac', 'fgr', 'sc2', 'clique'])
def test_default_poses_are_those_of_pair_by_pair_matching(dev, pairs, described, estimator):
    from buffer_amd import evaluate
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    d, seeds = described, [3, 4]
    reg = FpfhRegistration(THREEDMATCH, dev, estimator=estimator)
    assert reg.match_ratio is None
    poses = reg.register_batch(d['inps'], seeds)
    want = _poses_from(reg, d, d['corrs'], seeds, estimator)
    assert len(poses) == 2 and all(torch.equal(a, b) for a, b in zip(poses, want))
    assert torch.equal(reg.register_batch(d['inps'][1:], seeds[1:])[0], poses[1])        # alone as in the batch
    # with the ratio test: other matches, the poses still inside the DGR thresholds of the self-registration test
    thin = FpfhRegistration(THREEDMATCH, dev, estimator=estimator, match_ratio=RATIO)
    assert thin.match_ratio == RATIO
    for pose, (_, ref) in zip(thin.register_batch(d['inps'], seeds), pairs):
        ok, rte, rre = evaluate.dgr_success(pose.cpu().numpy(), ref, 0.3, 15.0)
        print(f'{estimator} with match_ratio {RATIO}: rte {rte:.3e} m, rre {rre:.3e} deg')
        assert ok, (rte, rre)


def test_driver_line_carries_match_ratio(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import threedmatch as tdm
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:1])           # one scene: three pairs
    _mini_dataset(root, tdm.SCENES, seed=5)
    args = ['--root', root, '--log-name', 'run.log', '--batch', '2', '--descriptor', 'fpfh', '--estimator', 'fgr']
    tdm.main(args + ['--log-root', str(tmp_path / 'thin'), '--match-ratio', '0.8'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out['descriptor'] == 'fpfh' and out['estimator'] == 'fgr' and out['match_ratio'] == 0.8 and out['pairs'] == 3
    tdm.main(args + ['--log-root', str(tmp_path / 'full')])
    assert 'match_ratio' not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_standin_correspondences_from_features(dev, described):
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import ops
    regm = o3d.pipelines.registration
    d = described
    off = d['off']
    fa, fb = d['F'][off[0]:off[1]], d['F'][off[1]:off[2]]
    sf, tf = regm.Feature(fa.cpu().numpy().T), regm.Feature(fb.cpu().numpy().T)
    forward = ops.feature_match(fa, [len(fa)], fb, [len(fb)], mutual=False)[0].cpu().numpy()
    mutual = ops.feature_match(fa, [len(fa)], fb, [len(fb)], mutual=True)[0].cpu().numpy()
    assert len(forward) == len(fa) and 0 < len(mutual) <= len(forward)
    got = regm.correspondences_from_features(sf, tf)
    assert got.dtype == np.int32 and np.array_equal(got, forward)
    assert np.array_equal(regm.correspondences_from_features(sf, tf, True, 0.0), mutual)
    assert np.array_equal(regm.correspondences_from_features(sf, tf, True), mutual if len(mutual) >= 0.1 * len(forward) else forward)
    # open3d's rule: too few mutual survivors -> the forward matches
    assert np.array_equal(regm.correspondences_from_features(sf, tf, True, 1.0 + 1.0 / len(forward)), forward)
    assert np.array_equal(mutual, d['corrs'][0].cpu().numpy())
