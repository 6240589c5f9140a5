"""Fast Global Registration above the kernel: FpfhRegistration(estimator='fgr') on the self-registration scene of
tests/test_fpfh_register_gpu.py, the open3d stand-in's registration_fast_based_on_feature_matching, and one test-set driver with
--descriptor fpfh --estimator fgr."""
import json
import os

import numpy as np
import pytest
import torch

from test_fpfh_register_gpu import _errors, _pair, _upload

pytestmark = pytest.mark.gpu

# Self-registration with estimator='fgr', measured on an MI355X against the float64 Kabsch pose of the true correspondences (printed
# by the test), pair 0 / pair 1:
#   FGR pose               rotation 1.099e-06 / 1.182e-06 degrees, translation 3.014e-08 / 3.593e-08 m
#   after point-to-plane   rotation 1.103e-06 / 1.202e-06 degrees, translation 3.014e-08 / 3.625e-08 m, fitness 1, 1 iteration each
# (fp64 least squares over ~1 900 exact correspondences: the error left is the fp32 rounding of the returned pose).  Each limit is 2 x the
# largest measurement.  More than 0.5 degrees or one voxel would be a finding.
MEASURED_RRE_DEG = 1.21e-6
MEASURED_RTE = 3.7e-8


@pytest.fixture(scope='module')
def pairs():
    return [_pair(11, 0.7), _pair(12, 2.1)]


def test_self_registration_with_fgr(dev, pairs):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    reg = FpfhRegistration(THREEDMATCH, dev, estimator='fgr')
    inps = [_upload(p, dev) for p, _ in pairs]
    poses = reg.register_batch(inps, [3, 4])
    assert len(poses) == 2 and all(p.shape == (4, 4) and p.dtype == torch.float32 and p.is_cuda for p in poses)
    ref_d = reg.refine_batch(inps, poses, method='point_to_plane', max_dist=0.1, max_iteration=30)
    before = [_errors(pose.cpu().numpy(), ref) for pose, (_, ref) in zip(poses, pairs)]
    after = [_errors(ref_d['poses'][b].cpu().numpy(), ref) for b, (_, ref) in enumerate(pairs)]
    for b in range(2):                                           # every figure is printed before anything is asserted on it
        print(f'FGR self-registration pair {b}: rotation error {before[b][0]:.3e} deg, translation error {before[b][1]:.3e} m; after '
              f'point-to-plane: {after[b][0]:.3e} deg, {after[b][1]:.3e} m, fitness {float(ref_d["fitness"][b]):.4f}, '
              f'{int(ref_d["iterations"][b])} iterations')
    assert 2 * MEASURED_RRE_DEG <= 0.5 and 2 * MEASURED_RTE <= THREEDMATCH.voxel_size_0
    for b in range(2):
        assert before[b][0] <= 2 * MEASURED_RRE_DEG and before[b][1] <= 2 * MEASURED_RTE, before[b]
        assert after[b][0] <= 2 * MEASURED_RRE_DEG and after[b][1] <= 2 * MEASURED_RTE, after[b]
        assert float(ref_d['fitness'][b]) == 1.0
    # a pair's pose does not depend on the batch, and a rerun gives the same bits
    assert torch.equal(reg.register_batch(inps[1:], [4])[0], poses[1]) and torch.equal(reg.register_batch(inps, [3, 4])[0], poses[0])
    assert reg.register_batch([]) == []
    # estimator='ransac' is what a registration built without the argument does, bit for bit
    a = FpfhRegistration(THREEDMATCH, dev, estimator='ransac').register_batch(inps, [3, 4])
    b = FpfhRegistration(THREEDMATCH, dev).register_batch(inps, [3, 4])
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], poses[0])
    with pytest.raises(ValueError):
        FpfhRegistration(THREEDMATCH, dev, estimator='teaser')


def test_open3d_standin_follows_the_library(dev, pairs):
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import fgr, fpfh
    from buffer_amd.config import THREEDMATCH
    regm = o3d.pipelines.registration
    p, ref = pairs[0]
    radius = 5.0 * THREEDMATCH.voxel_size_0
    clouds, feats = [], []
    for pts, nrm in ((p['src'], p['snr']), (p['tgt'], p['tnr'])):
        pcd = o3d.geometry.PointCloud()
        pcd.points, pcd.normals = o3d.utility.Vector3dVector(pts), o3d.utility.Vector3dVector(nrm)
        clouds.append(pcd)
        feats.append(regm.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(radius=radius, max_nn=100)))
    res = regm.registration_fast_based_on_feature_matching(clouds[0], clouds[1], feats[0], feats[1],
                                                           regm.FastGlobalRegistrationOption(maximum_correspondence_distance=0.025), seed=3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    corr = fpfh.match(t(feats[0].data.T), t(feats[1].data.T), True)
    want = fgr.fast_global_registration(t(p['src']), [len(p['src'])], t(p['tgt']), [len(p['tgt'])], corr, [int(corr.shape[0])], seeds=[3])
    assert int(want['status'][0]) == 1 and np.array_equal(res.transformation, want['poses'][0].cpu().numpy())
    rre, rte = _errors(res.transformation, ref)
    print(f'FGR stand-in: {rre:.3e} deg, {rte:.3e} m, fitness {res.fitness:.4f}, inlier_rmse {res.inlier_rmse:.3e}, '
          f'{len(res.correspondence_set)} of {int(corr.shape[0])} matches')
    assert rre <= 0.5 and rte <= THREEDMATCH.voxel_size_0
    assert res.fitness > 0.9 and len(res.correspondence_set) >= 3
    with pytest.raises(NotImplementedError):
        regm.registration_fast_based_on_feature_matching(clouds[0], clouds[1], feats[0], feats[1],
                                                         regm.FastGlobalRegistrationOption(use_absolute_scale=True))


def test_threedmatch_driver_with_the_fgr_estimator(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import threedmatch as tdm
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:2])           # two scenes: six pairs
    _mini_dataset(root, tdm.SCENES, seed=5)
    tdm.main(['--root', root, '--log-name', 'run.log', '--batch', '2', '--log-root', str(tmp_path / 'fgr'), '--descriptor', 'fpfh',
              '--estimator', 'fgr'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with capsys.disabled():                                      # recorded in DESIGN.md section 7, not asserted
        print('FPFH + FGR driver line:', {k: out[k] for k in ('pairs', 'dgr_recall', 'registration_recall', 'te', 're')})
    assert out['descriptor'] == 'fpfh' and out['estimator'] == 'fgr' and out['pairs'] == 6 and out['limits'] is None
    for k in ('dgr_recall', 'registration_recall', 'per_scene', 'te', 're', 'pairs_per_sec', 'n_gpus', 'preset'):
        assert k in out, k
    assert os.path.exists(os.path.join(str(tmp_path / 'fgr'), tdm.SCENES[0], 'run.log'))
