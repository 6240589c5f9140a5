"""The voxelized refinement stage on the device: BufferPipeline.refine_batch(method='voxelized'), driver.register_pairs(refine=) and
`buffer_amd.eth --refine voxelized`, on the synthetic ETH root of tests/test_gicp_refine_gpu.py (two scenes x three stations, 6 pairs).
What is asserted is plumbing: unrefined results keep their bits, the refined poses are those of a direct icp.vgicp_batched call.
Whether the refinement helps the recall of these synthetic pairs is printed, not asserted."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRESET = '3DMatch->ETH'
SCENES = ['gazebo_summer', 'wood_autmn']
REFINE = dict(method='voxelized', max_dist=None, max_iteration=10, epsilon=1e-3, voxel=0.5, neighbors=7)


@pytest.fixture(scope='module')
def eth_root(tmp_path_factory):
    from buffer_amd import synth
    root = str(tmp_path_factory.mktemp('eth_vgicp'))
    synth.make_eth_root(root, scenes=SCENES, stations=3, seed=5)
    return root


@pytest.fixture(scope='module')
def setup(eth_root, dev):
    """the data set and a pipeline with frozen limits"""
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


def test_voxelized_refine_leaves_the_unrefined_results_alone_and_equals_the_direct_call(setup, dev):
    from buffer_amd import driver, icp, preprocess
    cfg, ds, pipe = setup
    idx = list(range(len(ds)))
    plain, counts = driver.register_pairs(pipe, ds, idx, 3, stage_metrics=True)
    poses, counts_r, ref = driver.register_pairs(pipe, ds, idx, 3, stage_metrics=True, refine=REFINE)
    assert torch.equal(poses, plain) and torch.equal(counts_r, counts)
    assert ref['poses'].shape == (6, 4, 4) and ref['poses'].dtype == torch.float32 and ref['iterations'].dtype == torch.int32
    assert torch.isfinite(ref['poses']).all() and int(ref['iterations'].max()) <= REFINE['max_iteration']
    for lo in (0, 3):
        inps = [driver.upload(s) for s in driver.items_batched(ds, idx[lo:lo + 3], dev)]
        got = pipe.refine_batch(inps, [plain[i] for i in range(lo, lo + 3)], **REFINE)
        for k in ref:
            assert torch.equal(got[k], ref[k][lo:lo + 3]), (k, lo)
        srcs, tgts = [i['src_raw'] for i in inps], [i['tgt_raw'] for i in inps]
        sl, tl = [s.shape[0] for s in srcs], [t.shape[0] for t in tgts]
        nrm = preprocess.estimate_normals(torch.cat(srcs + tgts), knn=30, orient=False, lengths=sl + tl)
        sn, tn = list(torch.split(nrm[:sum(sl)], sl)), list(torch.split(nrm[sum(sl):], tl))
        inits = [plain[i].cpu().numpy().astype(np.float64) for i in range(lo, lo + 3)]
        for voxel, nb in ((REFINE['voxel'], 7), (None, 27)):               # voxel=None: twice the correspondence distance
            direct = icp.vgicp_batched(srcs, tgts, inits, sn, tn, voxel=2.0 * cfg.dist_th if voxel is None else voxel, epsilon=1e-3,
                                       neighbors=nb, max_iteration=10)
            got = pipe.refine_batch(inps, plain[lo:lo + 3], method='voxelized', max_iteration=10, voxel=voxel, neighbors=nb)
            for b, d in enumerate(direct):
                assert np.array_equal(got['poses'][b].cpu().numpy(), d['T'].astype(np.float32)), (nb, lo, b)
                assert float(got['fitness'][b]) == d['fitness'] and float(got['inlier_rmse'][b]) == d['inlier_rmse'], (nb, lo, b)
                assert int(got['iterations'][b]) == d['iterations'], (nb, lo, b)
            assert any(d['iterations'] > 0 for d in direct) and all(d['fitness'] > 0 for d in direct)
    with pytest.raises(ValueError):
        pipe.refine_batch(inps, plain[3:], method='colored')


def test_eth_driver_voxelized_flags(eth_root, dev, capsys):
    from buffer_amd import eth

    def main(extra, limits=None):
        lim = ['--limits', ','.join(map(str, limits))] if limits else []
        poses = eth.main(['--root', eth_root, '--preset', PRESET, '--batch', '3', '--scenes'] + SCENES + lim + list(extra))
        return poses, json.loads([ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith('{')][-1])
    p0, out0 = main(())
    p1, out1 = main(('--refine', 'voxelized', '--refine-voxel', '0.5', '--refine-neighbors', '27', '--refine-iters', '10'), out0['limits'])
    print('ETH_VGICP_REFINE ' + json.dumps(dict(unrefined={k: out0[k] for k in ('recall', 'te', 're')}, refined=out1['refined'])))
    assert np.array_equal(p0, p1)
    assert set(out1) == set(out0) | {'refined'}
    assert all(out1[k] == out0[k] or (out1[k] != out1[k] and out0[k] != out0[k]) for k in out0 if k != 'pairs_per_sec')   # (NaN te / re)
    r = out1['refined']
    assert r['pairs'] == 6 and r['method'] == 'voxelized' and r['voxel'] == 0.5 and r['neighbors'] == 27 and r['max_iteration'] == 10
    assert all(np.isfinite(r[k]) for k in ('recall', 'fitness', 'inlier_rmse', 'iterations', 'max_dist'))
    assert 0.0 <= r['fitness'] <= 1.0 and 0.0 <= r['iterations'] <= 10
