"""--denoise above the kernels: the 3DMatch driver on the mini data set of test_threedmatch_driver.py (one scene, three pairs), once as it
is and once with a few far points planted into every fragment and --denoise statistical."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANTED = 10


def _plant(root, seed):
    """append PLANTED points 1.5 - 3 m outside the box of every fragment -> {fragment id: f32[PLANTED,3]}"""
    from buffer_amd import threedmatch as tdm
    rng = np.random.default_rng(seed)
    out = {}
    for path in sorted(glob.glob(os.path.join(root, 'test', '3DMatch', 'fragments', '*', '*.ply'))):
        pts = tdm.read_ply(path).astype(np.float32)
        mn, mx = pts.min(0), pts.max(0)
        far = rng.uniform(mn, mx, (PLANTED, 3))
        axis, side = rng.integers(0, 3, PLANTED), rng.integers(0, 2, PLANTED)
        off = rng.uniform(1.5, 3.0, PLANTED)
        far[np.arange(PLANTED), axis] = np.where(side == 0, mn[axis] - off, mx[axis] + off)
        far = far.astype(np.float32)
        tdm.write_ply(path, np.concatenate([pts, far]))
        out[os.path.splitext(os.path.basename(path))[0]] = far
    return out


def _line(tdm, argv, capsys):
    poses = tdm.main(argv)
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1]), poses


def _nearest(a, b):
    return torch.cdist(a.double(), b.double()).min(1).values


def test_driver_with_and_without_denoise(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import driver, preprocess, threedmatch as tdm
    from buffer_amd import config
    from buffer_amd.pipeline import BufferPipeline
    from test_threedmatch_driver import _mini_dataset
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:1])           # one scene: three pairs
    root = str(tmp_path / 'data')
    _mini_dataset(root, tdm.SCENES, seed=5)
    common = ['--root', root, '--log-name', 'run.log', '--batch', '3']
    # without the option: no key, and the samples are those of the call without the argument
    plain, plain_poses = _line(tdm, common + ['--log-root', str(tmp_path / 'a')], capsys)
    assert 'denoise' not in plain and plain['pairs'] == 3
    ds = tdm.ThreeDMatchTestSet(root)
    raws = [torch.from_numpy(r).to(dev) for r in ds.raw_pair(0)]
    a = preprocess.prepare_fragments(raws, ds.downsample, ds.voxel_size_0, ds.max_num_pts, [0, 1])
    b = preprocess.prepare_fragments(raws, ds.downsample, ds.voxel_size_0, ds.max_num_pts, [0, 1], denoise=None)
    s = ds.item(0, dev)
    for i, side in enumerate(('src', 'tgt')):
        assert set(a[i]) == {'fds_pts', 'sds_pts'} == set(b[i])
        for k in ('fds_pts', 'sds_pts'):
            assert torch.equal(a[i][k], b[i][k]) and torch.equal(a[i][k], s[f'{side}_{k}'])
    # ... and the poses and the log are those of the registration written out on a data set that has no `denoise` attribute at all
    assert not hasattr(ds, 'denoise') and not hasattr(ds, 'denoise_log')
    pipe = BufferPipeline(config.PRESETS[config.DRIVER_PRESETS['threedmatch'][0]], dev)      # the driver's default preset
    pipe.limits = plain['limits']
    poses = tdm.register_pairs(pipe, ds, range(len(ds)), batch=3).cpu().numpy()
    assert np.array_equal(poses, plain_poses)
    tdm.write_logs(ds, poses, str(tmp_path / 'a2'), 'run.log')
    with open(tmp_path / 'a' / tdm.SCENES[0] / 'run.log') as f1, open(tmp_path / 'a2' / tdm.SCENES[0] / 'run.log') as f2:
        assert f1.read() == f2.read()

    # far points planted into every fragment
    planted = _plant(root, 77)
    ds = tdm.ThreeDMatchTestSet(root)
    src_id = os.path.basename(ds.files[0][0])
    far = torch.from_numpy(planted[src_id]).to(dev)
    dirty = ds.item(0, dev)
    assert float(_nearest(far, dirty['src_fds_pts']).max()) < 1e-4            # they survive the voxel levels ...
    ds.denoise, ds.denoise_log = dict(method='statistical', nb_neighbors=20, std_ratio=2.0), []
    clean = ds.item(0, dev)
    assert float(_nearest(far, clean['src_fds_pts']).min()) > 0.5             # ... and not the filter
    assert float(_nearest(far, clean['src_sds_pts'][:, :3]).min()) > 0.5
    assert len(ds.denoise_log) == 2 and all(0.0 < f < 0.2 for f in ds.denoise_log)
    n_dirty, n_clean = dirty['src_fds_pts'].shape[0], clean['src_fds_pts'].shape[0]
    assert n_dirty - n_clean >= PLANTED and n_dirty - n_clean == round(ds.denoise_log[0] * n_dirty)
    # the batched path gives the same samples as pair by pair
    both = driver.items_batched(ds, [0], dev)[0]
    assert all(torch.equal(both[k], clean[k]) for k in ('src_fds_pts', 'src_sds_pts', 'tgt_fds_pts', 'tgt_sds_pts'))

    out, _ = _line(tdm, common + ['--log-root', str(tmp_path / 'b'), '--denoise', 'statistical'], capsys)
    assert out['denoise']['method'] == 'statistical' and out['denoise']['nb_neighbors'] == 20 and out['denoise']['std_ratio'] == 2.0
    assert 0.0 < out['denoise']['removed'] < 0.2 and out['pairs'] == 3
    with capsys.disabled():
        for name, o in (('plain', plain), ('planted + statistical', out)):
            print(f'denoise driver line ({name}):', {k: o[k] for k in ('pairs', 'dgr_recall', 'registration_recall', 'te', 're', 'denoise') if k in o})
    # the pairs still register inside the driver's thresholds: no fewer than on the clean clouds
    assert out['dgr_recall'] >= plain['dgr_recall'] > 0 and out['registration_recall'] >= plain['registration_recall']
