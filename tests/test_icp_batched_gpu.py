"""On-device ICP (csrc/icp.hip, buffer_amd/icp.py): parity with a serial host restatement of the point-to-point loop, one exact
step against numpy, determinism, point-to-plane, edge cases, the open3d stand-in and the KITTI ground-truth cache."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


_SCENES = {}


def _scene(seed):
    from buffer_amd import synth
    if seed not in _SCENES:
        _SCENES[seed] = synth.make_pair(seed, n_raw=60_000, size=(1.2, 1.0, 0.9), n_boxes=3)['src_fds_pts'].astype(np.float64)
    return _SCENES[seed]


def _pair(seed, n_src, n_tgt, angle=1.5, shift=(0.03, -0.02, 0.015)):
    """target = a sample of a box scene, source = another sample moved by the inverse of a planted pose (R, t) inside ICP's basin."""
    pts = _scene(seed % 3)
    rng = np.random.default_rng(seed)
    tgt = pts[rng.permutation(len(pts))[:n_tgt]]
    R = _rot(*np.deg2rad([0.3 * angle, -0.5 * angle, angle]))
    t = np.array(shift)
    src = (pts[rng.permutation(len(pts))[:n_src]] - t) @ R                # R src + t lands on the scene
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src.astype(np.float32), tgt.astype(np.float32), T


def _dev_list(arrs, dev):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 3)).to(dev) for a in arrs]


def _six_pairs():
    sizes = [(2000, 3000), (5000, 4000), (9000, 12000), (15000, 20000)]
    srcs, tgts = [], []
    for k, (n, m) in enumerate(sizes):
        s, t, _ = _pair(10 + k, n, m)
        srcs.append(s); tgts.append(t)
    s, t, _ = _pair(20, 3000, 3000)
    srcs.append(s + np.float32(100.0)); tgts.append(t)                    # disjoint: no correspondence
    srcs.append(np.zeros((0, 3), np.float32)); tgts.append(_pair(21, 10, 4000)[1])   # empty source
    return srcs, tgts


def _kabsch_dev(p, q):
    """rigid T (4x4 f64, numpy) minimising sum |R p + t - q|^2; p, q f64[n,3] device tensors."""
    pc, qc = p.mean(0), q.mean(0)
    H = ((p - pc).T @ (q - qc)).cpu().numpy()
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = qc.cpu().numpy() - R @ pc.cpu().numpy()
    return T


def _serial(src, tgt, dist, init, k, rf, rr):
    """The reference: open3d's point-to-point loop on the host, one pair, three host round trips per iteration (nearest target
    point = column 0 of ops.CellGrid.query, torch fp64 sums, numpy Kabsch) -> (T, fitness, rmse, corr, updates)."""
    from buffer_amd import ops
    dev = src.device
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    n, m = int(src.shape[0]), int(tgt.shape[0])
    if n == 0 or m == 0:
        return T, 0.0, 0.0, np.zeros((0, 2), np.int32), 0
    grid = ops.CellGrid(tgt.float().contiguous(), [m], float(dist))
    src64, tgt64 = src.double(), tgt.double()

    def correspond(Tn):
        Tt = torch.from_numpy(Tn).to(dev)
        moved = src64 @ Tt[:3, :3].T + Tt[:3, 3]
        nn = grid.query(moved.float().contiguous(), [n], 1)[:, 0].long()
        hit = torch.nonzero(nn < m).flatten()
        if hit.numel() == 0:
            return moved, hit, nn, 0.0, 0.0
        d2 = ((moved[hit] - tgt64[nn[hit]]) ** 2).sum(1)
        return moved, hit, nn, hit.numel() / n, float(torch.sqrt(d2.mean()).item())

    moved, hit, nn, fit, rmse = correspond(T)
    updates = 0
    for _ in range(int(k)):
        if hit.numel() < 3:
            break
        T = _kabsch_dev(moved[hit], tgt64[nn[hit]]) @ T
        updates += 1
        prev_fit, prev_rmse = fit, rmse
        moved, hit, nn, fit, rmse = correspond(T)
        if abs(prev_fit - fit) < rf and abs(prev_rmse - rmse) < rr:
            break
    corr = torch.stack([hit, nn[hit]], 1).to(torch.int32).cpu().numpy() if hit.numel() else np.zeros((0, 2), np.int32)
    return T, float(fit), float(rmse), corr, updates


@pytest.mark.gpu
def test_parity_with_the_host_reference_point_to_point_loop(dev):
    from buffer_amd import icp
    srcs, tgts = _six_pairs()
    S, Tg = _dev_list(srcs, dev), _dev_list(tgts, dev)
    k = 6
    res = icp.icp_batched(S, Tg, 0.05, max_iteration=k, relative_fitness=0.0, relative_rmse=0.0)
    for b in range(6):
        T, fit, rmse, _, it = _serial(S[b], Tg[b], 0.05, None, k, 0.0, 0.0)
        assert res[b]['iterations'] == it, (b, res[b]['iterations'], it)
        assert np.abs(res[b]['T'] - T).max() < 1e-7, b
        assert abs(res[b]['fitness'] - fit) < 1e-12 and abs(res[b]['inlier_rmse'] - rmse) < 1e-9, b
    assert [r['iterations'] for r in res[:4]] == [k] * 4 and res[4]['iterations'] == 0 and res[5]['iterations'] == 0
    assert res[4]['fitness'] == 0.0 and np.array_equal(res[4]['T'], np.eye(4))
    assert res[5]['fitness'] == 0.0 and res[5]['inlier_rmse'] == 0.0 and np.array_equal(res[5]['T'], np.eye(4))
    res = icp.icp_batched(S, Tg, 0.05, max_iteration=60)                  # default convergence criteria
    for b in range(6):
        T, fit, rmse, _, it = _serial(S[b], Tg[b], 0.05, None, 60, 1e-6, 1e-6)
        assert np.abs(res[b]['T'] - T).max() < 1e-6, b
        assert abs(res[b]['fitness'] - fit) < 1e-3, b


def _moved(src, T):
    """the kernel's fp64 transform, rounded to fp32 for the search"""
    s = src.astype(np.float64)
    p = np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1)
    return p, p.astype(np.float32)


def _brute_nn(q32, tgt, dist):
    """nearest target point with fp32 d2 = ((dx*dx + dy*dy) + dz*dz) < r2 (strict), ties to the lowest index"""
    r2 = np.float32(dist) * np.float32(dist)
    out = np.full(len(q32), -1, np.int64)
    for lo in range(0, len(q32), 512):
        q = q32[lo:lo + 512]
        dx, dy, dz = (q[:, None, c] - tgt[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = np.where(d2 < r2, d2, np.float32(np.inf))
        j = np.argmin(d2, 1)                                              # first of the minima = lowest index
        out[lo:lo + 512] = np.where(np.isfinite(d2[np.arange(len(q)), j]), j, -1)
    return out


def _kabsch64(p, q):
    pc, qc = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - pc).T @ (q - qc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, qc - R @ pc
    return T


@pytest.mark.gpu
def test_one_exact_step_matches_numpy(dev):
    from buffer_amd import icp
    src, tgt, _ = _pair(31, 3000, 4000)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = _rot(0.002, -0.001, 0.003), [0.004, 0.002, -0.003]
    S, Tg = _dev_list([src], dev), _dev_list([tgt], dev)
    r0 = icp.icp_batched(S, Tg, 0.04, inits=[T0], max_iteration=0, return_correspondences=True)[0]
    p, q32 = _moved(src, T0)
    nn = _brute_nn(q32, tgt, 0.04)
    hit = np.flatnonzero(nn >= 0)
    assert hit.size > 100 and np.array_equal(r0['correspondences'], np.stack([hit, nn[hit]], 1))
    assert np.array_equal(r0['T'], T0) and r0['iterations'] == 0 and r0['fitness'] == hit.size / len(src)
    r1 = icp.icp_batched(S, Tg, 0.04, inits=[T0], max_iteration=1, return_correspondences=True)[0]
    want = _kabsch64(p[hit], tgt[nn[hit]].astype(np.float64)) @ T0
    assert r1['iterations'] == 1 and np.abs(r1['T'] - want).max() < 1e-10
    p1, q1 = _moved(src, r1['T'])
    nn1 = _brute_nn(q1, tgt, 0.04)
    h1 = np.flatnonzero(nn1 >= 0)
    assert np.array_equal(r1['correspondences'], np.stack([h1, nn1[h1]], 1))
    d2 = ((p1[h1] - tgt[nn1[h1]].astype(np.float64)) ** 2).sum(1)
    assert abs(r1['inlier_rmse'] - np.sqrt(d2.mean())) < 1e-12


@pytest.mark.gpu
def test_batch_composition_and_reruns_give_the_same_bits(dev):
    from buffer_amd import icp
    srcs, tgts = _six_pairs()
    S, Tg = _dev_list(srcs, dev), _dev_list(tgts, dev)
    a = icp.icp_batched(S, Tg, 0.05, max_iteration=40)
    b = icp.icp_batched(S, Tg, 0.05, max_iteration=40)
    for x, y in zip(a, b):
        assert np.array_equal(x['T'], y['T']) and x['fitness'] == y['fitness'] and x['inlier_rmse'] == y['inlier_rmse']
    for i in range(6):
        one = icp.icp_batched([S[i]], [Tg[i]], 0.05, max_iteration=40)[0]
        assert np.array_equal(one['T'], a[i]['T']) and one['fitness'] == a[i]['fitness'], i
        assert one['inlier_rmse'] == a[i]['inlier_rmse'] and one['iterations'] == a[i]['iterations'], i


def _normals(tgt, dev):
    from buffer_amd import preprocess
    return preprocess.estimate_normals(torch.from_numpy(tgt).to(dev), knn=30, orient=False).cpu().numpy()


@pytest.mark.gpu
def test_point_to_plane_one_step_matches_numpy(dev):
    from buffer_amd import icp
    src, tgt, _ = _pair(41, 4000, 6000)
    nrm = _normals(tgt, dev)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = _rot(0.003, 0.002, -0.004), [0.003, -0.004, 0.002]
    S, Tg, N = _dev_list([src], dev), _dev_list([tgt], dev), _dev_list([nrm], dev)
    r0 = icp.icp_batched(S, Tg, 0.05, [T0], 'point_to_plane', N, max_iteration=0, return_correspondences=True)[0]
    c = r0['correspondences']
    p, _ = _moved(src, T0)
    p, q, n = p[c[:, 0]], tgt[c[:, 1]].astype(np.float64), nrm[c[:, 1]].astype(np.float64)
    r = ((p - q) * n).sum(1)
    J = np.concatenate([np.cross(p, n), n], 1)
    x = np.linalg.solve(J.T @ J, -J.T @ r)
    dT = np.eye(4)
    dT[:3, :3], dT[:3, 3] = _rot(x[0], x[1], x[2]), x[3:]
    r1 = icp.icp_batched(S, Tg, 0.05, [T0], 'point_to_plane', N, max_iteration=1)[0]
    assert r1['iterations'] == 1 and np.abs(r1['T'] - dT @ T0).max() < 1e-8


@pytest.mark.gpu
def test_point_to_plane_recovers_a_planted_pose(dev):
    from buffer_amd import icp
    pts = _scene(1).astype(np.float32)
    rng = np.random.default_rng(3)
    R, t = _rot(*np.deg2rad([0.6, -0.8, 2.0])), np.array([0.02, -0.03, 0.01])
    src = ((pts[rng.permutation(len(pts))[:8000]].astype(np.float64) - t) @ R).astype(np.float32)
    nrm = _normals(pts, dev)
    T, fit, rmse, corr = icp.icp_point_to_plane(*_dev_list([src, pts, nrm], dev), 0.10, max_iteration=100)
    ang = np.arccos(np.clip((np.trace(T[:3, :3].T @ R) - 1) / 2, -1, 1))
    assert ang < 1e-4 and np.abs(T[:3, 3] - t).max() < 1e-4, (ang, T[:3, 3] - t)
    assert fit > 0.99 and len(corr) == round(fit * len(src))


@pytest.mark.gpu
def test_point_to_plane_with_too_few_matches_keeps_the_initial_pose(dev):
    from buffer_amd import icp
    _, tgt, _ = _pair(51, 5, 3000)
    src = tgt[:5].copy()                                                   # 5 exact matches: one short of a 6x6 system
    nrm = _normals(tgt, dev)
    T0 = np.eye(4)
    T0[:3, 3] = [0.001, 0.0, 0.0]
    T, fit, rmse, corr = icp.icp_point_to_plane(*_dev_list([src, tgt, nrm], dev), 0.05, init=T0)
    assert np.array_equal(T, T0) and len(corr) == 5


@pytest.mark.gpu
def test_edge_cases(dev):
    from buffer_amd import icp, _lib
    src, tgt, _ = _pair(61, 3000, 4000)
    src[::7] = np.nan
    src[3] = [np.inf, 0, 0]
    r = icp.icp_batched(*[[x] for x in _dev_list([src, tgt], dev)], 0.05, max_iteration=30, return_correspondences=True)[0]
    bad = np.flatnonzero(~np.isfinite(src).all(1))
    assert np.isfinite(r['T']).all() and r['iterations'] > 0 and r['fitness'] > 0.3
    assert not np.isin(r['correspondences'][:, 0], bad).any()
    torch.cuda.synchronize()
    S, Tg = _dev_list([src], dev), _dev_list([tgt], dev)
    for d in (0.0, -1.0):
        with pytest.raises(_lib.BufferHipError):
            icp.icp_batched(S, Tg, d)
    with pytest.raises(ValueError):
        icp.icp_batched(S, Tg, 0.05, method='point_to_plane')
    with pytest.raises(ValueError):
        icp.icp_batched(S, Tg, 0.05, method='point_to_plane', tgt_normals=_dev_list([tgt[:10]], dev))


@pytest.mark.gpu
def test_point_to_point_wrapper_edge_cases(dev):
    from buffer_amd import icp
    src, tgt, _ = _pair(62, 3000, 4000)
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, 0.0, 0.0]
    S, Tg = _dev_list([src, tgt], dev)
    for a, b in ((S[:0], Tg), (S, Tg[:0])):                               # empty source, empty target
        T, fit, rmse, corr = icp.icp_point_to_point(a, b, 0.05, T0)
        assert np.array_equal(T, T0) and fit == 0.0 and rmse == 0.0
        assert corr.shape == (0, 2) and corr.dtype == np.int32
    with pytest.raises(RuntimeError):
        icp.icp_point_to_point(torch.from_numpy(src), torch.from_numpy(tgt), 0.05)
    src[::5] = np.nan
    T, fit, rmse, corr = icp.icp_point_to_point(*_dev_list([src, tgt], dev), 0.05)
    assert np.isfinite(T).all() and fit > 0.3 and not np.isin(corr[:, 0], np.arange(0, len(src), 5)).any()


@pytest.mark.gpu
def test_open3d_standin_point_to_plane_and_point_to_point(dev):
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import icp
    reg = o3d.pipelines.registration
    src, tgt, _ = _pair(71, 6000, 8000)
    pcd0, pcd1 = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
    pcd0.points, pcd1.points = o3d.utility.Vector3dVector(src.astype(np.float64)), o3d.utility.Vector3dVector(tgt.astype(np.float64))
    with pytest.raises(RuntimeError, match="estimate_normals"):
        reg.registration_icp(pcd0, pcd1, 0.05, np.eye(4), reg.TransformationEstimationPointToPlane())
    pp = reg.registration_icp(pcd0, pcd1, 0.05, np.eye(4), reg.TransformationEstimationPointToPoint(),
                              reg.ICPConvergenceCriteria(max_iteration=50))
    T, fit, rmse, corr = icp.icp_point_to_point(*_dev_list([src, tgt], dev), 0.05, np.eye(4), 50)
    assert np.array_equal(pp.transformation, T) and pp.fitness == fit and pp.inlier_rmse == rmse
    assert np.array_equal(pp.correspondence_set, corr)
    pcd1.estimate_normals()
    res = reg.registration_icp(pcd0, pcd1, 0.05, np.eye(4), reg.TransformationEstimationPointToPlane(),
                               reg.ICPConvergenceCriteria(max_iteration=50))
    assert isinstance(res, reg.RegistrationResult)
    assert len(res.correspondence_set) == round(res.fitness * len(src)) and res.fitness > 0.9
    assert np.abs(res.transformation - pp.transformation).max() < 5e-3


@pytest.mark.gpu
def test_kitti_refine_ground_truths_matches_the_serial_refinement(tmp_path, dev):
    from test_kitti_driver import _mini_sequence
    from buffer_amd import kitti
    root = str(tmp_path / 'kitti')
    _mini_sequence(root)
    serial = kitti.KittiTestSet(root, drives=(8,))
    n = len(serial)
    want = []                                                              # the serial host refinement (_serial) of every pair
    for i in range(n):
        drive, t0, t1 = serial.files[i]
        p0, p1 = (kitti.odometry_to_positions(o) for o in serial.odometry(drive)[[t0, t1]])
        M = (kitti.VELO2CAM @ p0.T @ np.linalg.inv(p1.T) @ np.linalg.inv(kitti.VELO2CAM)).T
        xyz0 = serial.scan(drive, t0).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        T = _serial(*_dev_list([xyz0, serial.scan(drive, t1)], dev), 0.20, np.eye(4), 200, 1e-6, 1e-6)[0]
        want.append(M @ T)
    icp_dir = os.path.join(root, 'icp')
    one = [serial.ground_truth(i, dev) for i in range(n)]                  # a cache miss refines that pair alone
    assert all(serial.gt_source[i] == 'icp-device' for i in range(n))
    for i in range(n):
        assert np.array_equal(np.load(os.path.join(icp_dir, '%d_%d_%d.npy' % serial.files[i])), one[i]), i
    for f in os.listdir(icp_dir):
        os.remove(os.path.join(icp_dir, f))
    keep = os.path.join(icp_dir, '%d_%d_%d.npy' % serial.files[0])
    np.save(keep, np.eye(4))
    ds = kitti.KittiTestSet(root, drives=(8,))
    done = ds.refine_ground_truths(range(n), dev, batch=2)
    assert done == list(range(1, n))
    assert np.array_equal(np.load(keep), np.eye(4))                        # existing cache files are left alone
    for i in range(1, n):
        got = np.load(os.path.join(icp_dir, '%d_%d_%d.npy' % serial.files[i]))
        assert np.abs(got - want[i]).max() < 1e-6, i
        assert np.array_equal(got, one[i]), i                              # ground_truth() and a batch of 2 write the same bits
        assert ds.gt_source[i] == 'icp-device'
        assert np.array_equal(ds.ground_truth(i), got) and ds.gt_source[i] == 'icp-device'
    for f in os.listdir(icp_dir):
        os.remove(os.path.join(icp_dir, f))
    for drive in (9, 10):                                                  # the CLI reads all three test drives
        _mini_sequence(root, drive=drive, frames=14, seed=drive)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'buffer_amd.kitti', '--root', root, '--refine-gt', '--batch-icp', '2'], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for i in range(n):
        got = np.load(os.path.join(icp_dir, '%d_%d_%d.npy' % serial.files[i]))
        assert np.abs(got - want[i]).max() < 1e-6, i
    full = kitti.KittiTestSet(root)
    assert len(full) > n and all(os.path.exists(os.path.join(icp_dir, '%d_%d_%d.npy' % f)) for f in full.files)
