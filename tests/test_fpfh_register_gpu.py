"""The FPFH baseline above the kernel: FpfhRegistration on a synthetic scene registered onto a moved, permuted copy of itself, the
open3d stand-in's compute_fpfh_feature / registration_ransac_based_on_feature_matching, and one test-set driver with
--descriptor fpfh."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Self-registration, measured on an MI355X against the float64 Kabsch pose of the true correspondences (printed by the test):
#   RANSAC pose            rotation 7.157e-06 / 2.514e-06 degrees, translation 6.611e-08 / 6.144e-08 m (pair 0 / pair 1)
#   after point-to-plane   rotation 6.689e-06 / 2.010e-06 degrees, translation 4.185e-08 / 3.593e-08 m, fitness 1, 1 iteration each
# (a 3-point fp32 Kabsch on exact correspondences: fp32 round-off of the coordinates).  Each limit is 2 x the larger measurement; both are
# far inside the 3DMatch DGR thresholds (15 degrees, 0.3 m), which are the condition.
MEASURED_RRE_DEG = 7.2e-6
MEASURED_RTE = 6.7e-8


def _scene(seed, n=2000):
    """~n points on a floor carrying three unequal boxes (no symmetry), with the analytic normals of their faces"""
    rng = np.random.default_rng(seed)
    boxes = [(0.25, 0.20, 0.50, 0.35, 0.45), (1.10, 0.25, 0.30, 0.30, 0.80), (0.70, 0.90, 0.75, 0.30, 0.25)]     # x0, y0, w, d, h
    faces = [((0.0, 0.0, 0.0), (1.8, 0, 0), (0, 1.4, 0), (0, 0, 1.0))]                                                # origin, eu, ev, normal
    for x0, y0, w, d, h in boxes:
        faces += [((x0, y0, h), (w, 0, 0), (0, d, 0), (0, 0, 1.0)),
                  ((x0, y0, 0), (w, 0, 0), (0, 0, h), (0, -1.0, 0)), ((x0, y0 + d, 0), (w, 0, 0), (0, 0, h), (0, 1.0, 0)),
                  ((x0, y0, 0), (0, d, 0), (0, 0, h), (-1.0, 0, 0)), ((x0 + w, y0, 0), (0, d, 0), (0, 0, h), (1.0, 0, 0))]
    area = np.array([np.linalg.norm(np.cross(f[1], f[2])) for f in faces])
    pick = rng.choice(len(faces), size=4 * n, p=area / area.sum())
    uv = rng.random((4 * n, 2))
    o, eu, ev, nr = (np.array([faces[k][c] for k in pick], np.float64) for c in range(4))
    pts = o + uv[:, :1] * eu + uv[:, 1:] * ev
    under = np.zeros(len(pts), bool)                             # floor points under a box are not on the surface
    for x0, y0, w, d, h in boxes:
        under |= (pick == 0) & (pts[:, 0] > x0) & (pts[:, 0] < x0 + w) & (pts[:, 1] > y0) & (pts[:, 1] < y0 + d)
    keep = np.flatnonzero(~under)[:n]
    return pts[keep].astype(np.float32), nr[keep].astype(np.float32)


def _rigid(seed, angle):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    T[:3, 3] = rng.uniform(-1, 1, 3)
    return T


def _kabsch64(a, b):
    """float64 rigid transform a -> b over corresponding rows"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = cb - T[:3, :3] @ ca
    return T


def _errors(T, ref):
    """(rotation error in degrees, translation error) of T against ref; the angle from the Frobenius norm (exact for small angles)"""
    T, ref = np.asarray(T, np.float64), np.asarray(ref, np.float64)
    s = np.linalg.norm(T[:3, :3] - ref[:3, :3]) / (2 * math.sqrt(2))
    return 2 * math.asin(min(1.0, s)) * 180 / math.pi, float(np.linalg.norm(T[:3, 3] - ref[:3, 3]))


def _pair(seed, angle):
    """the scene and a permuted copy moved by a known transform -> (driver.upload-style dict, reference pose)"""
    pts, nrm = _scene(seed)
    T = _rigid(seed + 100, angle)
    perm = np.random.default_rng(seed + 200).permutation(len(pts))
    tgt = (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)[perm]
    tnr = (nrm.astype(np.float64) @ T[:3, :3].T).astype(np.float32)[perm]
    ref = _kabsch64(pts[perm], tgt)                              # the best pose for the rounded target: what the errors are measured against
    assert _errors(ref, T)[0] < 1e-4 and _errors(ref, T)[1] < 1e-5
    return dict(src=pts, snr=nrm, tgt=tgt, tnr=tnr), ref


def _upload(p, dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    return dict(points=torch.cat([t(p['src']), t(p['tgt'])]).contiguous(), features=torch.cat([t(p['snr']), t(p['tnr'])]).contiguous(),
                lengths=np.array([len(p['src']), len(p['tgt'])], np.int32), src_raw=t(p['src']), tgt_raw=t(p['tgt']))


@pytest.fixture(scope='module')
def pairs():
    return [_pair(11, 0.7), _pair(12, 2.1)]


def test_self_registration_meets_the_dgr_thresholds(dev, pairs):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    from buffer_amd import evaluate
    reg = FpfhRegistration(THREEDMATCH, dev)
    inps = [_upload(p, dev) for p, _ in pairs]
    poses = reg.register_batch(inps, [3, 4])
    assert len(poses) == 2 and all(p.shape == (4, 4) and p.dtype == torch.float32 and p.is_cuda for p in poses)
    out = reg.register_batches([inps], seeds=[[3, 4]], refine=dict(method='point_to_plane', max_dist=0.1, max_iteration=30))
    assert len(out) == 1 and len(out[0]) == 2
    res, ref_d = out[0]
    before = [_errors(pose.cpu().numpy(), ref) for pose, (_, ref) in zip(poses, pairs)]
    after = [_errors(ref_d['poses'][b].cpu().numpy(), ref) for b, (_, ref) in enumerate(pairs)]
    for b in range(2):                                           # every figure is printed before anything is asserted on it
        print(f'FPFH self-registration pair {b}: rotation error {before[b][0]:.3e} deg, translation error {before[b][1]:.3e} m; after '
              f'point-to-plane: {after[b][0]:.3e} deg, {after[b][1]:.3e} m, fitness {float(ref_d["fitness"][b]):.4f}, '
              f'{int(ref_d["iterations"][b])} iterations')
    for b, (pose, (_, ref)) in enumerate(zip(poses, pairs)):
        ok, rte, rre = evaluate.dgr_success(pose.cpu().numpy(), ref, 0.3, 15.0)
        assert ok, (rte, rre)                                    # the condition
        assert before[b][0] <= 2 * MEASURED_RRE_DEG and before[b][1] <= 2 * MEASURED_RTE, before[b]
    # a pair's pose does not depend on the batch, and a rerun gives the same bits
    alone = reg.register_batch(inps[1:], [4])
    assert torch.equal(alone[0], poses[1]) and torch.equal(reg.register_batch(inps, [3, 4])[0], poses[0])
    # refinement on the same clouds: the unrefined poses keep their bits, BufferPipeline.refine_batch's dict, and no larger error
    assert all(torch.equal(a, b) for a, b in zip(res, poses))
    assert sorted(ref_d) == ['fitness', 'inlier_rmse', 'iterations', 'poses']
    assert ref_d['poses'].shape == (2, 4, 4) and ref_d['poses'].dtype == torch.float32 and ref_d['fitness'].dtype == torch.float64
    assert ref_d['iterations'].dtype == torch.int32 and ref_d['inlier_rmse'].shape == (2,)
    for b in range(2):
        assert after[b][0] <= before[b][0] and after[b][1] <= before[b][1], (after[b], before[b])
        assert float(ref_d['fitness'][b]) == 1.0
    with pytest.raises(NotImplementedError):
        reg.register_batch(inps, [3, 4], metrics_gt=[np.eye(4)] * 2)
    with pytest.raises(NotImplementedError):
        reg.register_batches([inps], seeds=[[3, 4]], metrics_gt=[[np.eye(4)] * 2])
    assert reg.limits is None and reg.calibrate([]) is None
    # fewer than 3 matches: the identity
    tiny = dict(points=inps[0]['points'][:2].contiguous(), features=inps[0]['features'][:2].contiguous(), lengths=np.array([1, 1], np.int32))
    assert torch.equal(reg.register_batch([tiny], [0])[0], torch.eye(4, device=dev))
    assert reg.register_batch([]) == [] and reg.register_batches([]) == []


def test_open3d_standin_follows_the_library(dev, pairs):
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import fpfh
    from buffer_amd.config import THREEDMATCH
    regm = o3d.pipelines.registration
    p, ref = pairs[0]
    radius, dist = 5.0 * THREEDMATCH.voxel_size_0, 1.5 * THREEDMATCH.voxel_size_0
    clouds, feats = [], []
    for pts, nrm in ((p['src'], p['snr']), (p['tgt'], p['tnr'])):
        pcd = o3d.geometry.PointCloud()
        pcd.points, pcd.normals = o3d.utility.Vector3dVector(pts), o3d.utility.Vector3dVector(nrm)
        f = regm.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(radius=radius, max_nn=100))
        want = fpfh.compute_fpfh(torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev), radius, 100).cpu().numpy()
        assert f.dimension() == 33 and f.num() == len(pts) and f.data.dtype == np.float64 and np.array_equal(f.data, want.T)
        clouds.append(pcd)
        feats.append(f)
    res = regm.registration_ransac_based_on_feature_matching(
        clouds[0], clouds[1], feats[0], feats[1], True, dist, regm.TransformationEstimationPointToPoint(False), 3,
        [regm.CorrespondenceCheckerBasedOnEdgeLength(0.9), regm.CorrespondenceCheckerBasedOnDistance(dist)],
        regm.RANSACConvergenceCriteria(100000, 0.999), seed=3)
    pose = fpfh.FpfhRegistration(THREEDMATCH, dev).register_batch([_upload(p, dev)], [3])[0].cpu().numpy()
    assert np.array_equal(res.transformation, pose.astype(np.float64))
    assert res.fitness > 0.9 and res.inlier_rmse < dist and len(res.correspondence_set) >= 3
    with pytest.raises(NotImplementedError):
        regm.registration_ransac_based_on_feature_matching(clouds[0], clouds[1], feats[0], feats[1], True, dist, ransac_n=4)


def test_threedmatch_driver_with_the_fpfh_descriptor(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import threedmatch as tdm
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:2])           # two scenes: six pairs
    _mini_dataset(root, tdm.SCENES, seed=5)
    ds_args = ['--root', root, '--log-name', 'run.log', '--batch', '2']
    tdm.main(ds_args + ['--log-root', str(tmp_path / 'fpfh'), '--descriptor', 'fpfh', '--refine', 'point_to_plane'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with capsys.disabled():                                      # recorded in DESIGN.md section 7, not asserted
        print('FPFH driver line:', {k: out[k] for k in ('pairs', 'dgr_recall', 'registration_recall', 'te', 're')},
              'refined:', {k: out['refined'][k] for k in ('dgr_recall', 'registration_recall', 'te', 're', 'fitness')})
    assert out['descriptor'] == 'fpfh' and out['pairs'] == 6 and out['limits'] is None
    for k in ('dgr_recall', 'registration_recall', 'per_scene', 'te', 're', 'pairs_per_sec', 'n_gpus', 'preset', 'refined'):
        assert k in out, k
    assert out['refined']['method'] == 'point_to_plane' and 'fitness' in out['refined'] and 'dgr_recall' in out['refined']
    assert os.path.exists(os.path.join(str(tmp_path / 'fpfh'), tdm.SCENES[0], 'run.log'))
    tdm.main(ds_args + ['--log-root', str(tmp_path / 'buffer'), '--limits', '17,20,24'])
    base = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 'descriptor' not in base and base['pairs'] == 6 and base['limits'] == [17, 20, 24]
