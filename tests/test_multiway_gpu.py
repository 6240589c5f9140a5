"""python -m buffer_amd.multiway end to end on a 3DMatch-layout scene of five views of one synthetic room: the ten pairs go through
the registration pipeline, ONE pair's pose is replaced by a wrong one, and the pose graph has to switch exactly that edge off and
still place every fragment."""
import json
import os

import numpy as np
import pytest

import posegraph_ref as R

pytestmark = pytest.mark.gpu

OFFSETS = (0.0, 0.225, 0.45, 0.675, 0.9)
BAD = (1, 3)                                        # the pair whose pose is replaced (non-consecutive: the Registration Recall counts it)


def _five_views(seed, size=(2.4, 1.9, 1.7), width=1.5, n_raw=260_000):
    """slabs of one synth.make_scene room along x (the construction of the mini data set of tests/test_threedmatch_driver.py) ->
    (raw fragments f32[n,3], each in its own frame, poses fragment -> world)"""
    from buffer_amd import synth
    rng = np.random.default_rng(seed)
    rects = synth.make_scene(rng, size, 6)
    frags, world = [], []
    for lo in OFFSETS:
        pts, _ = synth.sample_scene(rng, rects, n_raw)
        pts = pts[(pts[:, 0] >= lo) & (pts[:, 0] <= lo + width)]
        sensor = np.array([lo + 0.5 * width, 0.55 * size[1], 0.5 * size[2]])
        Rm = synth.random_rotation(rng, 0.6)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rm, -Rm @ sensor
        world.append(np.linalg.inv(T))
        frags.append((pts @ Rm.T + T[:3, 3]).astype(np.float32))
    return frags, world


def test_one_wrong_pair_is_switched_off_and_every_fragment_is_placed(tmp_path, dev, capsys):
    from buffer_amd import evaluate, multiway, pairs, posegraph, threedmatch as tdm
    frags, W = _five_views(5)
    n, scene = len(frags), tdm.SCENES[0]
    root, log_root = str(tmp_path / 'data'), str(tmp_path / 'logs')
    frag_dir = os.path.join(root, 'test', '3DMatch', 'fragments', scene)
    for k, f in enumerate(frags):
        tdm.write_ply(os.path.join(frag_dir, f'cloud_bin_{k}.ply'), f)
        np.save(os.path.join(frag_dir, f'cloud_bin_{k}.pose.npy'), W[k])
    pairs.main(['--root', root, '--scene', scene])                                     # gt.log / gt.info from the pose.npy files
    capsys.readouterr()

    truth = np.linalg.inv(W[BAD[1]]) @ W[BAD[0]]                                        # source BAD[0] -> target BAD[1]
    wrong = truth @ R.random_motion(np.random.default_rng(35), 0.35, 0.3)
    assert not evaluate.dgr_success(wrong, truth, *tdm.DGR_THRESHOLDS)[0]
    ret = multiway.main(['--root', root, '--scenes', scene, '--all-pairs', '--min-overlap', '0', '--log-root', log_root, '--log-name', 'mw.log',
                         '--batch', '10'], override_poses={(scene, *BAD): wrong})
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(line)
    row = line['scenes'][scene]
    # the JSON line
    assert set(row) >= {'nodes', 'edges', 'dropped', 'pruned', 'solves', 'status', 'trajectory_rmse'}
    assert set(line['direct']) == set(line['optimized']) == {'registration_recall', 'dgr_recall'} and line['trajectory_rmse'] is not None
    assert row['nodes'] == n and line['pairs'] == 10 and row['edges'] + len(row['dropped']) == 10
    # exactly the corrupted edge is switched off
    off = {tuple(p) for p in row['dropped']} | {tuple(p) for p in row['pruned']}
    assert off == {BAD}, (row['dropped'], row['pruned'])
    assert all(s.startswith('CONVERGED') for s in row['status'])
    # every fragment within the driver's thresholds of its true pose relative to fragment 0
    err = posegraph.trajectory_error(ret[scene]['poses'], W, fixed=0)
    print('per-fragment RTE', err['rte'], 'RRE', err['rre'])
    assert err['rte'].max() < tdm.DGR_THRESHOLDS[0] and err['rre'].max() < tdm.DGR_THRESHOLDS[1]
    # the corrupted pair, read back from the trajectory, is right; its direct pose is not
    k = ret[scene]['pair_ids'].index(BAD)
    assert not evaluate.dgr_success(ret[scene]['direct_poses'][k], truth, *tdm.DGR_THRESHOLDS)[0]
    assert evaluate.dgr_success(ret[scene]['pair_poses'][k], truth, *tdm.DGR_THRESHOLDS)[0]
    assert line['optimized']['dgr_recall'] >= line['direct']['dgr_recall'] and line['optimized']['dgr_recall'] == 1.0
    # the files: the trajectory, and the pair log in the evaluator's format
    back = pairs.read_poses(os.path.join(log_root, scene, 'multiway_trajectory.log'), n, None)
    assert np.array_equal(np.array(back), ret[scene]['poses'])
    rr, per_scene = evaluate.registration_recall(os.path.join(root, 'test', '3DMatch', 'gt_result'), log_root, 'mw.log')
    assert 0.0 <= rr <= 1.0 and len(per_scene) == 1 and rr == pytest.approx(line['optimized']['registration_recall'], abs=1e-6)
    assert line['optimized']['registration_recall'] >= line['direct']['registration_recall']
