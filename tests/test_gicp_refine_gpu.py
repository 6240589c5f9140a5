"""The dense pose-refinement stage on the device: BufferPipeline.refine_batch, register_batches(refine=), driver.register_pairs(refine=)
and `buffer_amd.eth --refine`, on a synthetic ETH root of two scenes x three stations (6 pairs).  What is asserted is plumbing:
unrefined results keep their bits, the refined poses are those of direct icp.icp_batched calls.  Whether the refinement helps the
recall of these synthetic pairs is printed, not asserted."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRESET = '3DMatch->ETH'
SCENES = ['gazebo_summer', 'wood_autmn']
REFINE = dict(method='generalized', max_dist=None, max_iteration=10, epsilon=1e-3)


@pytest.fixture(scope='module')
def eth_root(tmp_path_factory):
    from buffer_amd import synth
    root = str(tmp_path_factory.mktemp('eth_refine'))
    synth.make_eth_root(root, scenes=SCENES, stations=3, seed=5)
    return root


_RUNS = {}


def _main(eth_root, extra, capsys):
    """eth.main on the fixture root -> (poses, its JSON line); once per argument list"""
    from buffer_amd import eth
    key = tuple(extra)
    if key not in _RUNS:
        lim = ['--limits', ','.join(map(str, _RUNS[()][1]['limits']))] if key else []
        poses = eth.main(['--root', eth_root, '--preset', PRESET, '--batch', '3', '--scenes'] + SCENES + lim + list(extra))
        _RUNS[key] = poses, json.loads([ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith('{')][-1])
    return _RUNS[key]


@pytest.fixture(scope='module')
def setup(eth_root, dev):
    """the data set, a pipeline with frozen limits and the two chunks of three pairs"""
    from buffer_amd import eth
    from buffer_amd.config import preset
    from buffer_amd.pipeline import BufferPipeline
    cfg = preset(PRESET, 'eth')
    ds = eth.ETHTestSet(eth_root, SCENES, downsample=cfg.downsample, voxel_size_0=cfg.voxel_size_0, max_num_pts=cfg.max_num_pts)
    assert len(ds) == 6
    pipe = BufferPipeline(cfg, dev)
    host = [{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in ds.item(0, dev).items()}]
    pipe.calibrate(host)
    return cfg, ds, pipe


def test_refine_leaves_the_unrefined_results_alone_and_equals_direct_icp(setup, dev):
    from buffer_amd import driver, icp, preprocess
    cfg, ds, pipe = setup
    idx = list(range(len(ds)))
    plain, counts = driver.register_pairs(pipe, ds, idx, 3, stage_metrics=True)
    poses, counts_r, ref = driver.register_pairs(pipe, ds, idx, 3, stage_metrics=True, refine=REFINE)
    assert torch.equal(poses, plain) and torch.equal(counts_r, counts)
    only, ref2 = driver.register_pairs(pipe, ds, idx, 3, refine=REFINE)                     # without the metric rows: the same again
    assert torch.equal(only, plain) and all(torch.equal(ref[k], ref2[k]) for k in ref)
    assert ref['poses'].shape == (6, 4, 4) and ref['poses'].dtype == torch.float32 and ref['poses'].is_cuda
    assert ref['fitness'].shape == (6,) and ref['inlier_rmse'].shape == (6,) and ref['iterations'].dtype == torch.int32
    assert torch.isfinite(ref['poses']).all() and int(ref['iterations'].max()) <= REFINE['max_iteration']
    for lo in (0, 3):
        inps = [driver.upload(s) for s in driver.items_batched(ds, idx[lo:lo + 3], dev)]
        got = pipe.refine_batch(inps, [plain[i] for i in range(lo, lo + 3)], **REFINE)
        for k in ref:
            assert torch.equal(got[k], ref[k][lo:lo + 3]), (k, lo)
        assert all(torch.equal(got[k], pipe.refine_batch(inps, plain[lo:lo + 3], **REFINE)[k]) for k in got)    # a [B,4,4] tensor
        srcs, tgts = [i['src_raw'] for i in inps], [i['tgt_raw'] for i in inps]
        sl = [s.shape[0] for s in srcs]
        nrm = preprocess.estimate_normals(torch.cat(srcs + tgts), knn=30, orient=False, lengths=sl + [t.shape[0] for t in tgts])
        sn, tn = list(torch.split(nrm[:sum(sl)], sl)), list(torch.split(nrm[sum(sl):], [t.shape[0] for t in tgts]))
        inits = [plain[i].cpu().numpy().astype(np.float64) for i in range(lo, lo + 3)]
        kw = dict(max_iteration=REFINE['max_iteration'])
        for method, extra in (('generalized', dict(src_normals=sn, tgt_normals=tn, epsilon=1e-3)), ('point_to_plane', dict(tgt_normals=tn)),
                              ('point_to_point', {})):
            direct = icp.icp_batched(srcs, tgts, cfg.dist_th, inits, method, **extra, **kw)
            got = pipe.refine_batch(inps, plain[lo:lo + 3], method=method, max_iteration=REFINE['max_iteration'])
            for b, d in enumerate(direct):
                assert np.array_equal(got['poses'][b].cpu().numpy(), d['T'].astype(np.float32)), (method, lo, b)
                assert float(got['fitness'][b]) == d['fitness'] and float(got['inlier_rmse'][b]) == d['inlier_rmse'], (method, lo, b)
                assert int(got['iterations'][b]) == d['iterations'], (method, lo, b)
    with pytest.raises(ValueError):
        pipe.refine_batch(inps, plain[3:], method='colored')
    empty = pipe.refine_batch([], [])
    assert empty['poses'].shape == (0, 4, 4) and empty['iterations'].shape == (0,)


def test_eth_driver_refine_flag(eth_root, dev, capsys):
    p0, out0 = _main(eth_root, (), capsys)
    p1, out1 = _main(eth_root, ('--refine', 'generalized', '--refine-iters', '10'), capsys)
    print('ETH_REFINE ' + json.dumps(dict(unrefined={k: out0[k] for k in ('recall', 'te', 're')}, refined=out1['refined'])))
    assert np.array_equal(p0, p1)
    assert set(out1) == set(out0) | {'refined'}
    assert all(out1[k] == out0[k] or (out1[k] != out1[k] and out0[k] != out0[k]) for k in out0 if k != 'pairs_per_sec')   # (NaN te / re)
    r = out1['refined']
    assert r['pairs'] == 6 and r['method'] == 'generalized' and r['max_iteration'] == 10
    assert {'recall', 'te', 're', 'per_scene', 'fitness', 'inlier_rmse', 'iterations', 'max_dist'} <= set(r)
    assert all(np.isfinite(r[k]) for k in ('recall', 'fitness', 'inlier_rmse', 'iterations', 'max_dist'))
    assert 0.0 <= r['fitness'] <= 1.0 and 0.0 <= r['iterations'] <= 10
    from buffer_amd import eth
    with pytest.raises(SystemExit):
        eth.main(['--root', eth_root, '--refine', 'colored'])
    capsys.readouterr()
