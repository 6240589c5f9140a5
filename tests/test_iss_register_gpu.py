"""The ISS keypoint mode of the FPFH baseline above the kernel: FpfhRegistration(keypoints='iss') on the floor-and-boxes scene of
test_fpfh_register_gpu.py registered onto a moved, permuted copy of itself, the open3d stand-in's compute_iss_keypoints and one
test-set driver with --descriptor fpfh --keypoints iss.

The scene carries Gaussian jitter (sigma = 0.002, default_rng(seed + 300)), added before the copy is made: on exact planes l3 is
rounding noise and a third of the points are undecided.  With it the restatement (tests/iss_ref.py) finds, at the default factors
(radii 0.21 / 0.14), 32 keypoints in each of the four clouds, 31 of 32 and 32 of 32 of them repeated in the moved copy, and 49 / 57 / 33 /
44 undecided points of 2000 (source, target of pair 0; source, target of pair 1): at most 2.85 %, under the cap of 5 % asserted
on the CPU before the device mask is compared on the decided points."""
import json
import math

import numpy as np
import pytest
import torch

import iss_ref
from test_fpfh_register_gpu import _errors, _kabsch64, _rigid, _scene, _upload

pytestmark = pytest.mark.gpu
SIGMA = 0.002
UNDECIDED_CAP = 0.05


def _pair(seed, angle):
    """the jittered scene and a permuted copy moved by a known transform -> (driver.upload-style dict, reference pose, permutation)"""
    pts, nrm = _scene(seed)
    pts = (pts + np.random.default_rng(seed + 300).normal(scale=SIGMA, size=pts.shape)).astype(np.float32)
    T = _rigid(seed + 100, angle)
    perm = np.random.default_rng(seed + 200).permutation(len(pts))
    tgt = (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)[perm]
    tnr = (nrm.astype(np.float64) @ T[:3, :3].T).astype(np.float32)[perm]
    ref = _kabsch64(pts[perm], tgt)
    assert _errors(ref, T)[0] < 1e-4 and _errors(ref, T)[1] < 1e-5
    return dict(src=pts, snr=nrm, tgt=tgt, tnr=tnr), ref, perm


@pytest.fixture(scope='module')
def pairs():
    return [_pair(11, 0.7), _pair(12, 2.1)]


@pytest.fixture(scope='module')
def radii():
    from buffer_amd.config import THREEDMATCH
    return 6.0 * THREEDMATCH.voxel_size_0, 4.0 * THREEDMATCH.voxel_size_0


@pytest.fixture(scope='module')
def restated(pairs, radii):
    """the restatement on the four clouds, once: [(mask, undecided)] in the order src0, tgt0, src1, tgt1"""
    out = []
    for p, _, _ in pairs:
        for pts in (p['src'], p['tgt']):
            r = iss_ref.iss(pts, iss_ref.radius_rows(pts, radii[0]), iss_ref.radius_rows(pts, radii[1]))
            out.append((r['mask'], r['undecided']))
    return out


def _proper_rigid(T):
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    return (np.isfinite(T).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-4 and abs(np.linalg.det(R) - 1.0) < 1e-4
            and np.array_equal(T[3], [0, 0, 0, 1]))


def test_device_mask_equals_the_restatement_on_the_decided_points(dev, pairs, radii, restated):
    from buffer_amd import keypoints
    und = [int(u.sum()) for _, u in restated]
    kps = [int(m.sum()) for m, _ in restated]
    print(f'ISS scene: keypoints {kps}, undecided {und} of 2000')
    assert all(u <= UNDECIDED_CAP * 2000 for u in und), und      # on the CPU first: a wrong input, not a tolerance
    assert kps == [32, 32, 32, 32] and und[0] == 49 and und[2] == 33
    for b, (p, _, perm) in enumerate(pairs):                     # repeatability of the restatement's keypoints under the motion
        src_kp, tgt_kp = set(np.flatnonzero(restated[2 * b][0])), set(perm[np.flatnonzero(restated[2 * b + 1][0])])
        print(f'ISS scene pair {b}: {len(src_kp & tgt_kp)} of {len(src_kp)} keypoints repeated in the moved copy')
        assert len(src_kp & tgt_kp) == (31, 32)[b]
    clouds = [c for p, _, _ in pairs for c in (p['src'], p['tgt'])]
    stacked = torch.from_numpy(np.concatenate(clouds)).to(dev)
    lens = [len(c) for c in clouds]
    idx, counts = keypoints.iss_keypoints(stacked, radii[0], radii[1], lengths=lens)
    mask = np.zeros(sum(lens), np.uint8)
    mask[idx.cpu().numpy()] = 1
    lo = 0
    for c, (want, undecided) in enumerate(restated):
        got = mask[lo:lo + lens[c]]
        differ = np.flatnonzero(got != want)
        print(f'ISS scene cloud {c}: {int(got.sum())} device keypoints, {len(differ)} points differ from the restatement (all undecided: '
              f'{bool(undecided[differ].all())})')
        assert np.array_equal(got[~undecided], want[~undecided]), differ
        assert counts[c] == int(got.sum())
        lo += lens[c]


def test_iss_registration_meets_the_dgr_thresholds(dev, pairs):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    from buffer_amd import evaluate, keypoints
    reg = FpfhRegistration(THREEDMATCH, dev, keypoints='iss')
    inps = [_upload(p, dev) for p, _, _ in pairs]
    poses = reg.register_batch(inps, [3, 4])
    counts = reg.keypoint_counts.copy()
    assert len(poses) == 2 and all(p.shape == (4, 4) and p.dtype == torch.float32 and p.is_cuda for p in poses)
    errs = [_errors(pose.cpu().numpy(), ref) for pose, (_, ref, _) in zip(poses, pairs)]
    for b in range(2):                                           # printed and recorded, not a limit
        print(f'ISS registration pair {b}: {counts[2 * b]} / {counts[2 * b + 1]} keypoints, rotation error {errs[b][0]:.3e} deg, '
              f'translation error {errs[b][1]:.3e} m')
    for pose, (_, ref, _) in zip(poses, pairs):
        ok, rte, rre = evaluate.dgr_success(pose.cpu().numpy(), ref, 0.3, 15.0)
        assert ok, (rte, rre)                                    # the condition: the DGR thresholds
    # keypoint_counts is what iss_keypoints gives on the same stacked clouds
    pts = torch.cat([i['points'] for i in inps]).float().contiguous()
    lens = np.concatenate([i['lengths'] for i in inps])
    idx, want = keypoints.iss_keypoints(pts, reg.iss_salient_radius, reg.iss_non_max_radius, lengths=lens)
    assert counts.dtype == np.int64 and np.array_equal(counts, want) and int(counts.sum()) == len(idx) and (counts > 0).all()
    assert reg.iss_salient_radius == 6.0 * THREEDMATCH.voxel_size_0 and reg.iss_non_max_radius == 4.0 * THREEDMATCH.voxel_size_0
    # a pair's pose does not depend on the batch, and a rerun gives the same bits
    alone = reg.register_batch(inps[1:], [4])
    assert torch.equal(alone[0], poses[1]) and np.array_equal(reg.keypoint_counts, counts[2:])
    again = reg.register_batch(inps, [3, 4])
    assert torch.equal(again[0], poses[0]) and torch.equal(again[1], poses[1])
    # refinement goes on on the dense clouds
    out = reg.register_batches([inps], seeds=[[3, 4]], refine=dict(method='point_to_plane', max_dist=0.1, max_iteration=30))
    res, ref_d = out[0]
    assert all(torch.equal(a, b) for a, b in zip(res, poses)) and ref_d['poses'].shape == (2, 4, 4)
    for b, (_, ref, _) in enumerate(pairs):
        after = _errors(ref_d['poses'][b].cpu().numpy(), ref)
        print(f'ISS registration pair {b} after point-to-plane on the dense clouds: {after[0]:.3e} deg, {after[1]:.3e} m, '
              f'fitness {float(ref_d["fitness"][b]):.4f}')
        assert float(ref_d['fitness'][b]) > 0.99                 # every dense source point finds its partner: the whole clouds were used
    # fewer than 3 matches: the identity
    tiny = dict(points=inps[0]['points'][:2].contiguous(), features=inps[0]['features'][:2].contiguous(), lengths=np.array([1, 1], np.int32))
    assert torch.equal(reg.register_batch([tiny], [0])[0], torch.eye(4, device=dev)) and reg.keypoint_counts.tolist() == [0, 0]
    with pytest.raises(ValueError):
        FpfhRegistration(THREEDMATCH, dev, keypoints='harris')


@pytest.mark.parametrize('estimator', ['fgr', 'sc2', 'clique'])
def test_the_other_estimators_run_on_the_keypoint_matches(dev, pairs, estimator):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    reg = FpfhRegistration(THREEDMATCH, dev, estimator=estimator, keypoints='iss')
    inps = [_upload(p, dev) for p, _, _ in pairs]
    poses = reg.register_batch(inps, [3, 4])
    assert len(poses) == 2 and reg.keypoint_counts.shape == (4,)
    for b, (pose, (_, ref, _)) in enumerate(zip(poses, pairs)):
        T = pose.cpu().numpy()
        e = _errors(T, ref)
        print(f'ISS + {estimator} pair {b}: rotation error {e[0]:.3e} deg, translation error {e[1]:.3e} m (printed, not asserted: about 30 '
              f'matches are outside what this estimator was tuned on)')
        assert pose.shape == (4, 4) and pose.dtype == torch.float32 and _proper_rigid(T), T


def test_keypoints_none_is_the_default_path_bit_for_bit(dev, pairs):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    inps = [_upload(p, dev) for p, _, _ in pairs]
    default, none = FpfhRegistration(THREEDMATCH, dev), FpfhRegistration(THREEDMATCH, dev, keypoints=None)
    a, b = default.register_batch(inps, [3, 4]), none.register_batch(inps, [3, 4])
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and default.keypoint_counts is None and none.keypoint_counts is None
    for (_, ref, _), pose in zip(pairs, a):
        assert _errors(pose.cpu().numpy(), ref)[0] < 15.0


def test_open3d_standin_returns_the_rows_of_iss_keypoints(dev, pairs, radii):
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import keypoints, ops
    p = pairs[0][0]
    pcd = o3d.geometry.PointCloud()
    pcd.points, pcd.normals = o3d.utility.Vector3dVector(p['src']), o3d.utility.Vector3dVector(p['snr'])
    t = torch.from_numpy(p['src']).to(dev)
    kp = o3d.geometry.keypoint.compute_iss_keypoints(pcd, salient_radius=radii[0], non_max_radius=radii[1])
    idx = keypoints.iss_keypoints(t, radii[0], radii[1])[0].cpu().numpy()
    assert len(idx) >= 3 and np.array_equal(np.asarray(kp.points), p['src'][idx].astype(np.float64)) and kp.has_normals()
    assert np.array_equal(np.asarray(kp.normals), p['snr'][idx].astype(np.float64))
    # zero radii: 6 x / 4 x the mean nearest-neighbour distance
    res = float(ops.knn(t[None], t[None], 2)[0][0, :, 1].double().mean())
    assert 0.005 < res < 0.05
    kp0 = o3d.geometry.keypoint.compute_iss_keypoints(pcd)
    idx0 = keypoints.iss_keypoints(t, 6.0 * res, 4.0 * res)[0].cpu().numpy()
    assert np.array_equal(np.asarray(kp0.points), p['src'][idx0].astype(np.float64))
    bare = o3d.geometry.PointCloud(p['src'])
    assert not o3d.geometry.keypoint.compute_iss_keypoints(bare, radii[0], radii[1]).has_normals()


def test_threedmatch_driver_with_iss_keypoints(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import threedmatch as tdm
    from buffer_amd.config import THREEDMATCH
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:2])           # two scenes: six pairs
    _mini_dataset(root, tdm.SCENES, seed=5)
    tdm.main(['--root', root, '--log-name', 'run.log', '--batch', '2', '--log-root', str(tmp_path / 'iss'), '--descriptor', 'fpfh',
              '--keypoints', 'iss'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with capsys.disabled():                                      # recorded in DESIGN.md, not asserted
        print('ISS driver line:', {k: out[k] for k in ('pairs', 'dgr_recall', 'registration_recall', 'te', 're', 'keypoints')})
    assert out['descriptor'] == 'fpfh' and out['estimator'] == 'ransac' and out['pairs'] == 6
    kp = out['keypoints']
    assert kp['detector'] == 'iss' and kp['salient_radius'] == 6.0 * THREEDMATCH.voxel_size_0
    assert kp['non_max_radius'] == 4.0 * THREEDMATCH.voxel_size_0 and math.isfinite(kp['mean_per_cloud']) and kp['mean_per_cloud'] >= 0
