"""The max-clique + TLS estimator above the kernel: FpfhRegistration(estimator='clique') on the self-registration scene of
tests/test_fpfh_register_gpu.py, held to that file's pose limits, and one test-set driver with --descriptor fpfh --estimator clique."""
import json
import os

import pytest
import torch

from test_fpfh_register_gpu import MEASURED_RRE_DEG, MEASURED_RTE, _errors, _pair, _upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pairs():
    return [_pair(11, 0.7), _pair(12, 2.1)]


def test_self_registration_with_the_clique_estimator(dev, pairs):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.fpfh import FpfhRegistration
    reg = FpfhRegistration(THREEDMATCH, dev, estimator='clique')
    assert reg.certified is None and reg.bound is None
    inps = [_upload(p, dev) for p, _ in pairs]
    poses = reg.register_batch(inps, [3, 4])
    assert len(poses) == 2 and all(p.shape == (4, 4) and p.dtype == torch.float32 and p.is_cuda for p in poses)
    err = [_errors(pose.cpu().numpy(), ref) for pose, (_, ref) in zip(poses, pairs)]
    for b in range(2):                                           # every figure is printed before anything is asserted on it
        print(f'clique self-registration pair {b}: rotation error {err[b][0]:.3e} deg, translation error {err[b][1]:.3e} m, bound '
              f'{int(reg.bound[b])}, certified {bool(reg.certified[b])}')
    for b in range(2):
        assert err[b][0] <= 2 * MEASURED_RRE_DEG and err[b][1] <= 2 * MEASURED_RTE, err[b]
    assert reg.certified.shape == (2,) and reg.certified.dtype == torch.bool and reg.bound.shape == (2,) and int(reg.bound.min()) >= 3
    # no sampler: the seeds change nothing; a pair's pose does not depend on the batch, and a rerun gives the same bits
    assert torch.equal(reg.register_batch(inps, [8, 9])[0], poses[0]) and torch.equal(reg.register_batch(inps)[1], poses[1])
    assert torch.equal(reg.register_batch(inps[1:], [4])[0], poses[1]) and reg.certified.shape == (1,)
    assert reg.register_batch([]) == []
    # estimator='ransac' is what a registration built without the argument does, bit for bit
    a = FpfhRegistration(THREEDMATCH, dev, estimator='ransac').register_batch(inps, [3, 4])
    b = FpfhRegistration(THREEDMATCH, dev).register_batch(inps, [3, 4])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        FpfhRegistration(THREEDMATCH, dev, estimator='teaser')


def test_threedmatch_driver_with_the_clique_estimator(tmp_path, dev, capsys, monkeypatch):
    from buffer_amd import threedmatch as tdm
    from test_threedmatch_driver import _mini_dataset
    root = str(tmp_path / 'data')
    monkeypatch.setattr(tdm, 'SCENES', tdm.SCENES[:2])           # two scenes: six pairs
    _mini_dataset(root, tdm.SCENES, seed=5)
    tdm.main(['--root', root, '--log-name', 'run.log', '--batch', '2', '--log-root', str(tmp_path / 'clique'), '--descriptor', 'fpfh',
              '--estimator', 'clique'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with capsys.disabled():                                      # recorded in DESIGN.md, not asserted
        print('FPFH + clique driver line:', {k: out[k] for k in ('pairs', 'dgr_recall', 'registration_recall', 'te', 're', 'certified_pairs')})
    assert out['descriptor'] == 'fpfh' and out['estimator'] == 'clique' and out['pairs'] == 6 and out['limits'] is None
    assert isinstance(out['certified_pairs'], int) and 0 <= out['certified_pairs'] <= 6
    for k in ('dgr_recall', 'registration_recall', 'per_scene', 'te', 're', 'pairs_per_sec', 'n_gpus', 'preset'):
        assert k in out, k
    assert os.path.exists(os.path.join(str(tmp_path / 'clique'), tdm.SCENES[0], 'run.log'))
