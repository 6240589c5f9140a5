"""The hybrid normals above the kernel: BufferPipeline.refine_batch(normals='hybrid') and FpfhRegistration(normals='hybrid') on the
jittered floor-and-boxes scene of test_iss_register_gpu.py (registered onto a moved, permuted copy of itself; poses against the float64
Kabsch pose of the true correspondences, under the DGR thresholds 0.3 m / 15 deg), the defaults bit for bit against the same calls
written out as they were before the option existed, and the drivers' new keys on the mini data set of test_threedmatch_driver.py.
Errors and angles are printed and recorded, not limits."""
import json

import numpy as np
import pytest
import torch

from test_fpfh_register_gpu import _errors, _upload
from test_iss_register_gpu import _pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pairs():
    return [_pair(11, 0.7), _pair(12, 2.1)]


def _nudged(ref, seed, deg=3.0, shift=0.03):
    """the reference pose moved by `deg` degrees about a random axis and `shift` metres: where a refinement starts"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    D[:3, 3] = shift * ax
    return D @ ref


def _bare_pipeline(dev):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.pipeline import BufferPipeline
    pipe = BufferPipeline.__new__(BufferPipeline)                # refine_batch reads the device and the configuration only
    pipe.device, pipe.cfg = dev, THREEDMATCH
    return pipe


def test_refine_batch_with_hybrid_normals(dev, pairs):
    from buffer_amd import evaluate, preprocess
    pipe = _bare_pipeline(dev)
    inps = [_upload(p, dev) for p, _, _ in pairs]
    starts = torch.from_numpy(np.stack([_nudged(ref, 40 + b) for b, (_, ref, _) in enumerate(pairs)])).to(dev)
    for b, (_, ref, _) in enumerate(pairs):
        e = _errors(starts[b].cpu().numpy(), ref)
        print(f'hybrid refine pair {b} start: rotation error {e[0]:.3e} deg, translation error {e[1]:.3e} m')
    # the hybrid normals against the scene's analytic ones (unoriented: the angle between the lines)
    src = torch.cat([i['src_raw'] for i in inps]).float().contiguous()
    lens = [int(i['src_raw'].shape[0]) for i in inps]
    hyb = preprocess.estimate_normals_radius(src, 2.0 * pipe.cfg.dist_th, 30, orient=False, lengths=lens).cpu().numpy().astype(np.float64)
    knn = preprocess.estimate_normals(src, knn=30, orient=False, lengths=lens).cpu().numpy().astype(np.float64)
    true = np.concatenate([p['snr'] for p, _, _ in pairs]).astype(np.float64)
    for name, nrm in (('hybrid', hyb), ('30-NN', knn)):
        ang = np.degrees(np.arccos(np.clip(np.abs((nrm * true).sum(1)), 0.0, 1.0)))
        print(f'{name} normals against the analytic ones: median {np.median(ang):.3f} deg, 99th percentile {np.percentile(ang, 99):.3f} deg')
    for method in ('generalized', 'voxelized', 'point_to_plane'):
        got = pipe.refine_batch(inps, starts, method=method, normals='hybrid')
        base = pipe.refine_batch(inps, starts, method=method)
        assert got['poses'].shape == (2, 4, 4) and got['poses'].dtype == torch.float32 and got['poses'].is_cuda
        for b, (_, ref, _) in enumerate(pairs):
            e, e0 = _errors(got['poses'][b].cpu().numpy(), ref), _errors(base['poses'][b].cpu().numpy(), ref)
            print(f'hybrid refine {method} pair {b}: rotation error {e[0]:.3e} deg, translation error {e[1]:.3e} m, fitness '
                  f'{float(got["fitness"][b]):.4f}, {int(got["iterations"][b])} iterations (30-NN normals: {e0[0]:.3e} deg, {e0[1]:.3e} m)')
            ok, rte, rre = evaluate.dgr_success(got['poses'][b].cpu().numpy(), ref, 0.3, 15.0)
            assert ok, (method, b, rte, rre)                     # the condition: the DGR thresholds
        again = pipe.refine_batch(inps, starts, method=method, normals='hybrid', normal_radius=2.0 * pipe.cfg.dist_th, normal_max_nn=30)
        assert all(torch.equal(got[k], again[k]) for k in got)   # the defaults of the option, spelled out; and a rerun
    wide = pipe.refine_batch(inps, starts, method='generalized', normals='hybrid', normal_radius=0.3, normal_max_nn=60)
    assert torch.isfinite(wide['poses']).all()
    with pytest.raises(ValueError, match='unknown normals'):
        pipe.refine_batch(inps, starts, normals='pca')


def test_refine_batch_default_is_todays_call_bit_for_bit(dev, pairs):
    from buffer_amd import ops, preprocess
    pipe = _bare_pipeline(dev)
    inps = [_upload(p, dev) for p, _, _ in pairs]
    starts = torch.from_numpy(np.stack([_nudged(ref, 40 + b) for b, (_, ref, _) in enumerate(pairs)])).to(dev)
    got = pipe.refine_batch(inps, starts, method='generalized')
    # the call as refine_batch made it before it had a `normals` argument
    srcs, tgts = [i['src_raw'][:, :3] for i in inps], [i['tgt_raw'][:, :3] for i in inps]
    sl, tl = np.array([s.shape[0] for s in srcs], np.int32), np.array([t.shape[0] for t in tgts], np.int32)
    src, tgt = torch.cat(srcs).float().contiguous(), torch.cat(tgts).float().contiguous()
    nrm = preprocess.estimate_normals(torch.cat([src, tgt]), knn=30, orient=False, lengths=np.concatenate([sl, tl]))
    snrm, tnrm = nrm[:src.shape[0]].contiguous(), nrm[src.shape[0]:].contiguous()
    T, fit, rmse, iters, _ = ops.icp_batched(src, sl, tgt, tl, float(pipe.cfg.dist_th), starts.to(torch.float64).contiguous(), 'generalized',
                                             tnrm, 30, src_normals=snrm, epsilon=1e-3)
    assert torch.equal(got['poses'], T.float()) and torch.equal(got['fitness'], fit) and torch.equal(got['inlier_rmse'], rmse)
    assert torch.equal(got['iterations'], iters)
    assert all(torch.equal(got[k], pipe.refine_batch(inps, starts, method='generalized', normals='knn')[k]) for k in got)


def test_fpfh_registration_with_hybrid_normals(dev, pairs):
    from buffer_amd import evaluate, fpfh, ops, preprocess
    from buffer_amd.config import THREEDMATCH
    reg = fpfh.FpfhRegistration(THREEDMATCH, dev, normals='hybrid')
    assert reg.normal_radius == 2.0 * THREEDMATCH.voxel_size_0 and reg.normal_max_nn == 30
    inps = [_upload(p, dev) for p, _, _ in pairs]
    poses = reg.register_batch(inps, [3, 4])
    for b, (pose, (_, ref, _)) in enumerate(zip(poses, pairs)):
        e = _errors(pose.cpu().numpy(), ref)
        print(f'FPFH on hybrid normals pair {b}: rotation error {e[0]:.3e} deg, translation error {e[1]:.3e} m')
        ok, rte, rre = evaluate.dgr_success(pose.cpu().numpy(), ref, 0.3, 15.0)
        assert ok, (b, rte, rre)
    # what it computed: the normals of estimate_normals_radius (on any grid that covers the radius), then the default path on those normals
    pts = torch.cat([i['points'] for i in inps]).float().contiguous()
    lens = np.concatenate([i['lengths'] for i in inps])
    grid = ops.CellGrid(pts, lens, max(reg.radius, reg.normal_radius))
    nrm = preprocess.estimate_normals_radius(pts, reg.normal_radius, 30, lengths=lens, grid=grid)
    assert torch.equal(nrm, preprocess.estimate_normals_radius(pts, reg.normal_radius, 30, lengths=lens))
    assert bool(((nrm.double() * -pts.double()).sum(1) >= 0).all())                          # oriented to the origin
    given = [dict(i, features=n) for i, n in zip(inps, torch.split(nrm, [int(i['points'].shape[0]) for i in inps]))]
    want = fpfh.FpfhRegistration(THREEDMATCH, dev).register_batch(given, [3, 4])
    assert all(torch.equal(a, b) for a, b in zip(poses, want))
    alone = reg.register_batch(inps[1:], [4])                    # a pair's pose does not depend on the batch
    assert torch.equal(alone[0], poses[1])
    # keypoint mode
    kp = fpfh.FpfhRegistration(THREEDMATCH, dev, normals='hybrid', keypoints='iss')
    kposes = kp.register_batch(inps, [3, 4])
    want = fpfh.FpfhRegistration(THREEDMATCH, dev, keypoints='iss').register_batch(given, [3, 4])
    assert all(torch.equal(a, b) for a, b in zip(kposes, want)) and (kp.keypoint_counts > 0).all()
    # its refinement estimates the dense clouds' normals the same way
    for method in ('point_to_plane', 'generalized', 'point_to_point'):
        ref_d = reg.refine_batch(inps, poses, method=method, max_dist=0.1)
        want_d = fpfh.FpfhRegistration(THREEDMATCH, dev).refine_batch(given, poses, method=method, max_dist=0.1)
        assert all(torch.equal(ref_d[k], want_d[k]) for k in ref_d), method
        for b, (_, ref, _) in enumerate(pairs):
            e = _errors(ref_d['poses'][b].cpu().numpy(), ref)
            print(f'FPFH on hybrid normals pair {b} after {method}: rotation error {e[0]:.3e} deg, translation error {e[1]:.3e} m, fitness '
                  f'{float(ref_d["fitness"][b]):.4f}')
            assert evaluate.dgr_success(ref_d['poses'][b].cpu().numpy(), ref, 0.3, 15.0)[0]


def test_fpfh_registration_default_is_todays_call_bit_for_bit(dev, pairs):
    from buffer_amd import fpfh
    from buffer_amd.config import THREEDMATCH
    inps = [_upload(p, dev) for p, _, _ in pairs]
    reg = fpfh.FpfhRegistration(THREEDMATCH, dev)
    assert reg.normals == 'given'
    got = reg.register_batch(inps, [3, 4])
    # the calls as register_batch made them before it had a `normals` argument
    pts = torch.cat([i['points'] for i in inps]).float().contiguous()
    nrm = torch.cat([i['features'][:, :3] for i in inps]).float().contiguous()
    lens = np.concatenate([np.asarray(i['lengths'], np.int32).reshape(2) for i in inps])
    F = fpfh.compute_fpfh(pts, nrm, reg.radius, reg.max_nn, lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    corr, cl = fpfh.match_batch(F, lens, True, None)
    co = np.concatenate([[0], np.cumsum(cl)])
    for b in range(2):
        s0, t0, t1 = int(off[2 * b]), int(off[2 * b + 1]), int(off[2 * b + 2])
        want = fpfh.ransac_on_matches(pts[s0:t0], pts[t0:t1], corr[int(co[b]):int(co[b + 1])], THREEDMATCH.ransac_hypotheses, [3, 4][b],
                                      reg.max_dist, reg.edge_similarity)
        assert torch.equal(got[b], want)
    assert all(torch.equal(a, b) for a, b in zip(got, fpfh.FpfhRegistration(THREEDMATCH, dev, normals='given').register_batch(inps, [3, 4])))


def _driver_line(tdm, argv, capsys):
    tdm.main(argv)
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_threedmatch_driver_keys(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import threedmatch as tdm
    from buffer_amd.config import THREEDMATCH
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:1])           # one scene: three pairs
    _mini_dataset(root, tdm.SCENES, seed=5)
    common = ['--root', root, '--log-name', 'run.log', '--batch', '3']
    out = _driver_line(tdm, common + ['--log-root', str(tmp_path / 'a'), '--descriptor', 'fpfh', '--fpfh-normals', 'hybrid',
                                      '--refine', 'point_to_plane'], capsys)
    assert out['descriptor'] == 'fpfh' and out['fpfh_normals'] == 'hybrid' and out['pairs'] == 3 and 'refine_normals' not in out
    assert out['refined']['method'] == 'point_to_plane' and 'refine_normal_radius' not in out['refined']
    plain = _driver_line(tdm, common + ['--log-root', str(tmp_path / 'b'), '--descriptor', 'fpfh'], capsys)
    assert 'fpfh_normals' not in plain and 'refine_normals' not in plain
    learned = _driver_line(tdm, common + ['--log-root', str(tmp_path / 'c'), '--refine', 'generalized', '--refine-iters', '10',
                                          '--refine-normals', 'hybrid'], capsys)
    assert learned['refine_normals'] == 'hybrid' and learned['refined']['refine_normal_radius'] == 2.0 * THREEDMATCH.dist_th
    assert 'fpfh_normals' not in learned and learned['pairs'] == 3
    with capsys.disabled():                                      # recorded in DESIGN.md, not asserted
        for name, o in (('fpfh hybrid', out), ('fpfh given', plain), ('learned, refine hybrid', learned)):
            print(f'normals driver line ({name}):', {k: o[k] for k in ('pairs', 'dgr_recall', 'registration_recall', 'te', 're') if k in o},
                  {k: o['refined'][k] for k in ('dgr_recall', 'te', 're', 'fitness') if 'refined' in o and k in o['refined']})
