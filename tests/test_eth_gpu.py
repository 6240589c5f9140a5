"""The ETH driver and the cross-dataset presets on the device: `python -m buffer_amd.eth` end to end on a synthetic ETH root
(both presets, batch-invariant poses equal to direct pipeline calls), HIP vs the CPU oracle at the ETH constants
(0.15 m pyramid over outdoor scans, 1 m patches over the 0.05 m level, VN offsets scaled by 5 and by 0.5), and the
3DMatch->KITTI / KITTI->3DLoMatch presets through the existing drivers."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ETH_PRESETS = ['3DMatch->ETH', 'KITTI->ETH']
JSON_KEYS = {'pairs', 'recall', 'te', 're', 'per_scene', 'preset', 'pairs_per_sec', 'n_gpus', 'limits'}


@pytest.fixture(scope='module')
def eth_root(tmp_path_factory):
    """the four scenes, four stations each (24 pairs); three NaN / inf rows planted in every scan"""
    from buffer_amd import eth, synth
    root = str(tmp_path_factory.mktemp('eth'))
    synth.make_eth_root(root, scenes=eth.SCENES, stations=4, seed=11, non_finite_rows=3)
    return root


def _run(mod, argv, capsys):
    poses = mod.main(argv)
    out = json.loads([ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith('{')][-1])
    return poses, out


_ETH_RUNS = {}


def _eth_run(eth_root, name, capsys):
    """eth.main --preset name --batch 4 on the fixture root, once per preset for the tests below"""
    from buffer_amd import eth
    if name not in _ETH_RUNS:
        _ETH_RUNS[name] = _run(eth, ['--root', eth_root, '--preset', name, '--batch', '4'], capsys)
    return _ETH_RUNS[name]


def _direct(cfg, ds, limits, dev, chunks):
    """BufferPipeline(preset).register_batch on threedmatch.items_batched samples, chunk by chunk"""
    from buffer_amd.pipeline import BufferPipeline
    from buffer_amd.threedmatch import items_batched, upload
    pipe = BufferPipeline(cfg, dev, limits=limits)
    out = []
    for ch in chunks:
        out += [p.cpu().numpy() for p in pipe.register_batch([upload(s) for s in items_batched(ds, ch, dev)], seeds=ch)]
    return np.stack(out)


@pytest.mark.parametrize('name', ETH_PRESETS)
def test_eth_driver_end_to_end(eth_root, dev, capsys, name):
    """eth.main in-process: one JSON line; --batch 1 and --batch 4 give the same bits, and those of direct register_batch calls"""
    from buffer_amd import eth
    from buffer_amd.config import preset
    cfg = preset(name, 'eth')
    p4, out = _eth_run(eth_root, name, capsys)
    assert set(out) == JSON_KEYS and out['preset'] == name and out['pairs'] == 24 and out['n_gpus'] == 1, out
    assert set(out['per_scene']) == set(eth.SCENES) and len(out['limits']) == 3 and out['pairs_per_sec'] > 0
    lim = ','.join(map(str, out['limits']))
    p1, out1 = _run(eth, ['--root', eth_root, '--preset', name, '--batch', '1', '--limits', lim], capsys)
    assert np.array_equal(p1, p4), np.abs(p1 - p4).max()
    assert out1['recall'] == out['recall'] and out1['limits'] == out['limits']
    ds = eth.ETHTestSet(eth_root, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
    direct = _direct(cfg, ds, out['limits'], dev, [list(range(len(ds)))])
    assert np.array_equal(direct, p4), np.abs(direct - p4).max()
    assert eth.summarize(ds, direct)['recall'] == out['recall']
    # a scene subset registers those pairs only (its pair seeds are its own positions, so its poses are not compared bit for bit)
    ps, sub = _run(eth, ['--root', eth_root, '--preset', name, '--scenes', 'wood_autmn', '--limits', lim], capsys)
    assert sub['pairs'] == 6 and set(sub['per_scene']) == {'wood_autmn'} and ps.shape == (6, 4, 4) and np.isfinite(ps).all()


# DGR recall (RTE < 0.3 m, RRE < 2 deg, ThreeD2ETH/test.py:65-72) of the 24 synthetic pairs of `eth_root`.  There is no published
# figure for this synthetic set; the only source is the measurement on an MI355X below (poses bit-identical run to run, and equal
# to the CPU oracle in test_eth_hip_equals_cpu_oracle).  The synthetic scans are far harder than the real ETH set (one third of the
# second level kept, volumetric canopy noise, no pose refinement), so the figures are low; the wood scenes fail almost everywhere.
# Each bound sits two pairs below the measurement: a regression that costs pairs fails, a pair at the edge of the criterion does not.
RECALL_MEASURED = {'3DMatch->ETH': 5 / 24, 'KITTI->ETH': 3 / 24}
RECALL_BOUND = {'3DMatch->ETH': 3 / 24, 'KITTI->ETH': 1 / 24}


@pytest.mark.parametrize('name', ETH_PRESETS)
def test_eth_recall_bound(eth_root, dev, capsys, name):
    _, out = _eth_run(eth_root, name, capsys)
    print(f'ETH_RECALL {name}: ' + json.dumps(out) + f' (measured when the bound was set: {RECALL_MEASURED[name]:.4f})')
    assert out['recall'] >= RECALL_BOUND[name] - 1e-12, out


# (preset, data-set index of the pair): two pairs at 3DMatch->ETH (a gazebo and a wood scene), one at KITTI->ETH
PARITY = [('3DMatch->ETH', 1), ('3DMatch->ETH', 14), ('KITTI->ETH', 20)]


def test_eth_hip_equals_cpu_oracle(eth_root, dev, oracle):
    """The same prepared host sample (device pre-processing of the ETH driver, copied to the host) and the same limits through the
    HIP path and through oracle.pipeline_ref.register_pair in CPU child processes (tests/eth_oracle_worker.py), 1500 keypoints:
    keypoints identical, mutual matches identical up to 2 per pair (two descriptors tied to fp32 round-off, as in
    test_kitti_gpu.py), pose within 1e-4 (rotation entries; translation relative to the scan extent of tens of metres)."""
    from buffer_amd import eth
    from buffer_amd.config import preset
    from buffer_amd.pipeline import BufferPipeline
    from buffer_amd.threedmatch import items_batched
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tempfile.mkdtemp(prefix='buf_eth_')
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    threads = max(1, min(16, os.cpu_count() or 4) // len(PARITY))
    workers, got = [], []
    for w, (name, i) in enumerate(PARITY):
        cfg = replace(preset(name, 'eth'), num_keypts=1500)
        ds = eth.ETHTestSet(eth_root, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
        s = items_batched(ds, [i], dev)[0]
        host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
        pipe = BufferPipeline(cfg, dev)
        limits = pipe.calibrate([host])
        rng = np.random.default_rng(i)
        perms = [rng.permutation(len(host['src_fds_pts'])), rng.permutation(len(host['tgt_fds_pts']))]
        inp, out = os.path.join(tmp, f'in_{w}.npz'), os.path.join(tmp, f'out_{w}.npz')
        np.savez(inp, preset=name, keypts=1500, seed=i, limits=np.array(limits), perm0=perms[0], perm1=perms[1],
                 **{k: host[k] for k in ('src_fds_pts', 'tgt_fds_pts', 'src_sds_pts', 'tgt_sds_pts', 'relt_pose')})
        cmd = [sys.executable, os.path.join(root, 'tests', 'eth_oracle_worker.py'), '--inp', inp, '--out', out, '--threads', str(threads)]
        workers.append((subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT), out))
        pose, d = pipe.register(pipe.upload(host), seed=i, perms=[torch.from_numpy(p).to(dev) for p in perms], detail=True)
        got.append(dict(name=name, pair=i, limits=limits, pose=pose.cpu().numpy().astype(np.float64), kp=[k.cpu().numpy() for k in d['kpts']],
                        smids=d['s_mids'].cpu().numpy(), tmids=d['t_mids'].cpu().numpy(),
                        n=[len(host['src_sds_pts']), len(host['tgt_sds_pts']), len(host['src_fds_pts']), len(host['tgt_fds_pts'])],
                        extent=float(np.abs(host['src_fds_pts']).max())))
    rows = []
    for g, (p, out) in zip(got, workers):
        log = p.communicate(timeout=1500)[0].decode()
        assert p.returncode == 0, log[-3000:]
        want = np.load(out)
        assert np.array_equal(g['kp'][0], want['kp0']) and np.array_equal(g['kp'][1], want['kp1']), f'{g["name"]} pair {g["pair"]}: keypoints differ'
        sym = len(set(zip(g['smids'].tolist(), g['tmids'].tolist())) ^ set(zip(want['smids'].tolist(), want['tmids'].tolist())))
        wp = want['pose']
        rows.append(dict(preset=g['name'], pair=g['pair'], limits=g['limits'], points=g['n'], matches=int(len(g['smids'])),
                         matches_differing=sym, dR=float(np.abs(g['pose'][:3, :3] - wp[:3, :3]).max()),
                         dt=float(np.abs(g['pose'][:3, 3] - wp[:3, 3]).max()), extent=g['extent']))
    shutil.rmtree(tmp, ignore_errors=True)
    print('ETH_PARITY ' + json.dumps(rows))
    for r in rows:
        assert r['matches_differing'] <= 2, r
        if r['matches_differing'] == 0:
            assert r['dR'] < 1e-4 and r['dt'] < 1e-4 * r['extent'], r


def test_kitti_driver_3dmatch_to_kitti_preset(tmp_path, dev, capsys):
    """python -m buffer_amd.kitti --preset 3DMatch->KITTI (generalization/ThreeD2KITTI) on mini sequences of test_kitti_driver:
    the poses of direct BufferPipeline(THREEDMATCH_TO_KITTI) calls, scored at 0.3 m / 1 deg"""
    from test_kitti_driver import _mini_sequence
    from buffer_amd import kitti
    from buffer_amd.config import THREEDMATCH_TO_KITTI as cfg
    root = str(tmp_path / 'kitti')
    for drive in kitti.TEST_DRIVES:
        _mini_sequence(root, drive=drive, frames=26, seed=drive)
    poses, out = _run(kitti, ['--root', root, '--preset', '3DMatch->KITTI', '--allow-odometry-gt', '--batch', '2'], capsys)
    print('KITTI_PRESET ' + json.dumps(out))
    assert out['preset'] == '3DMatch->KITTI' and out['gt_source']['odometry'] == out['pairs'] == len(poses) > 0
    ds = kitti.KittiTestSet(root, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts,
                            allow_odometry_gt=True)
    idx = list(range(len(ds)))
    direct = _direct(cfg, ds, out['limits'], dev, [idx[lo:lo + 2] for lo in range(0, len(idx), 2)])
    assert np.array_equal(direct, poses), np.abs(direct - poses).max()
    again = kitti.summarize(ds, direct)
    assert again['recall'] == out['recall'] and again['pairs'] == out['pairs']


def test_threedmatch_driver_kitti_to_3dlomatch_preset(tmp_path, dev, capsys):
    """python -m buffer_amd.threedmatch --preset KITTI->3DLoMatch (generalization/KITTI2ThreeD: KITTI weights, keypts_th = 0,
    scale 0.035 / 0.30) on the mini set of test_threedmatch_driver, its gt files mirrored into the 3DLoMatch layout: the
    poses of direct BufferPipeline(KITTI_TO_3DLOMATCH) calls, the .log files (inverse poses, file order) and RR as for the default"""
    from test_threedmatch_driver import _mini_dataset
    from buffer_amd import evaluate, threedmatch as tdm
    from buffer_amd.config import KITTI_TO_3DLOMATCH as cfg
    root = str(tmp_path / 'data')
    _mini_dataset(root, tdm.SCENES, seed=5)
    for scene in tdm.SCENES:
        shutil.copytree(os.path.join(root, 'test', '3DMatch', 'gt_result', scene), os.path.join(root, 'test', '3DLoMatch', scene))
    log_root = str(tmp_path / 'logs')
    poses, out = _run(tdm, ['--root', root, '--preset', 'KITTI->3DLoMatch', '--log-root', log_root, '--log-name', 'x.log', '--batch', '8'],
                      capsys)
    print('3DLOMATCH_PRESET ' + json.dumps(out))
    assert out['preset'] == 'KITTI->3DLoMatch' and out['pairs'] == 24 and {'dgr_recall', 'registration_recall', 'per_scene'} <= set(out)
    ds = tdm.ThreeDMatchTestSet(root, '3DLoMatch', downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
    direct = _direct(cfg, ds, out['limits'], dev, [list(range(lo, lo + 8)) for lo in range(0, 24, 8)])
    assert np.array_equal(direct, poses), np.abs(direct - poses).max()
    for k, scene in enumerate(tdm.SCENES):
        keys, traj = evaluate.read_trajectory(os.path.join(log_root, scene, 'x.log'))
        assert [tuple(x[:2]) for x in keys] == [('0', '1'), ('0', '2'), ('1', '2')]
        for r in range(3):
            np.testing.assert_allclose(np.linalg.inv(traj[r].astype(np.float64)), poses[3 * k + r], rtol=0, atol=1e-4)
    rr, per_scene = evaluate.registration_recall(ds.gt_root, log_root, 'x.log')
    assert out['registration_recall'] == rr and out['per_scene'] == per_scene
