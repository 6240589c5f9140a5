"""buffer_amd/driver.py, the parts that need no device: the DGR summary on planted tables, the common command line of the three
drivers, and the chunking of register_pairs against a stub pipeline that records what register_batches is handed."""
import argparse
import math

import numpy as np
import pytest

COMMON = ('root', 'preset', 'batch', 'limits', 'stage_metrics', 'log_root', 'by_overlap')


def test_dgr_summary_planted_tables():
    from buffer_amd import driver
    out = driver.dgr_summary([(True, 0.1, 1.0), (True, 0.3, 3.0)])
    assert out == dict(pairs=2, recall=1.0, te=pytest.approx(0.2, abs=1e-15), re=pytest.approx(2.0, abs=1e-15))
    out = driver.dgr_summary([(True, 0.1, 1.0), (False, 9.0, 90.0), (False, 5.0, 50.0), (True, 0.2, 2.0)], 'dgr_recall')
    assert list(out) == ['pairs', 'dgr_recall', 'te', 're']
    assert out['pairs'] == 4 and out['dgr_recall'] == 0.5                       # the failures' errors stay out of te / re
    assert out['te'] == pytest.approx(0.15, abs=1e-15) and out['re'] == pytest.approx(1.5, abs=1e-15)
    out = driver.dgr_summary(np.array([[0, 9.0, 90.0], [0, 5.0, 50.0]]))
    assert out['pairs'] == 2 and out['recall'] == 0.0 and math.isnan(out['te']) and math.isnan(out['re'])
    for empty in ([], np.zeros((0, 3))):
        out = driver.dgr_summary(empty)
        assert out['pairs'] == 0 and out['recall'] == 0.0 and math.isnan(out['te']) and math.isnan(out['re'])


def test_common_options_are_the_same_on_all_three_parsers():
    from buffer_amd import config as C, driver, eth, kitti, threedmatch
    ap = argparse.ArgumentParser()
    driver.add_common_args(ap, 'eth', 8, 'log_ETH')
    assert tuple(a.dest for a in ap._actions if a.dest != 'help') == COMMON
    argv = ['--root', 'r', '--batch', '3', '--limits', '1,2,3', '--stage-metrics', '--log-root', 'x', '--by-overlap']
    for name, mod in (('threedmatch', threedmatch), ('kitti', kitti), ('eth', eth)):
        a, cfg = mod.parse_args(argv)
        assert [getattr(a, k) for k in COMMON] == ['r', C.DRIVER_PRESETS[name][0], 3, '1,2,3', True, 'x', True]
        assert cfg is C.PRESETS[C.DRIVER_PRESETS[name][0]]
        a, _ = mod.parse_args(['--root', 'r'])
        assert [getattr(a, k) for k in COMMON[3:]] == [None, False, None, False]


class _Pipe:
    """register_batches records its arguments and answers one pose per seed without evaluating a maker"""

    def __init__(self):
        import torch
        self.device = torch.device('cpu')
        self.calls = []

    def register_batches(self, batches, seeds=None, metrics_gt=None):
        import torch
        self.calls.append((batches, seeds, metrics_gt))
        poses = [[torch.eye(4) * (s + 1) for s in ch] for ch in seeds]
        if metrics_gt is None:
            return poses
        return [(ps, torch.full((len(ps), 7), ch[0], dtype=torch.int32)) for ps, ch in zip(poses, seeds)]


class _Set:
    def meta(self, index, device=None):
        return {'relt_pose': np.eye(4) * index}


def test_register_pairs_chunks_and_empty_input():
    torch = pytest.importorskip("torch")
    from buffer_amd import driver
    ids = [5, 9, 2, 7, 11, 3, 8]
    pipe = _Pipe()
    poses = driver.register_pairs(pipe, _Set(), iter(ids), 3)
    (makers, seeds, gts), = pipe.calls                                           # ONE register_batches call for all chunks
    assert seeds == [[5, 9, 2], [7, 11, 3], [8]] and gts is None
    assert len(makers) == 3 and all(callable(m) for m in makers)
    assert poses.shape == (7, 4, 4) and poses[:, 0, 0].tolist() == [i + 1 for i in ids]       # in the order of `indices`
    pipe = _Pipe()
    poses, counts = driver.register_pairs(pipe, _Set(), ids, 3, stage_metrics=True)
    (makers, seeds, gts), = pipe.calls
    assert seeds == [[5, 9, 2], [7, 11, 3], [8]] and len(makers) == len(gts) == 3
    assert [[g[0, 0] for g in gt()] for gt in gts] == seeds                     # each chunk's ground truth, made when asked for
    assert poses.shape == (7, 4, 4) and counts.dtype == torch.int32 and counts[:, 0].tolist() == [5, 5, 5, 7, 7, 7, 8]
    # nothing to do: empty results of the right shape, type and device
    pipe = _Pipe()
    poses = driver.register_pairs(pipe, _Set(), [], 3)
    assert poses.shape == (0, 4, 4) and poses.dtype == torch.float32 and poses.device == pipe.device
    poses, counts = driver.register_pairs(pipe, _Set(), [], 3, stage_metrics=True)
    assert poses.shape == (0, 4, 4) and poses.dtype == torch.float32
    assert counts.shape == (0, 7) and counts.dtype == torch.int32 and counts.device == pipe.device
    assert [c[:2] for c in pipe.calls] == [([], []), ([], [])]


def test_module_register_pairs_are_the_shared_one_at_their_default_batch():
    pytest.importorskip("torch")
    from buffer_amd import eth, kitti, threedmatch
    ids = list(range(40))
    for mod, batch in ((threedmatch, 32), (kitti, 4), (eth, 32)):
        pipe = _Pipe()
        poses = mod.register_pairs(pipe, _Set(), ids)
        assert [len(ch) for ch in pipe.calls[0][1]] == [batch] * (40 // batch) + [40 % batch] * (40 % batch > 0)
        assert poses[:, 0, 0].tolist() == [i + 1 for i in ids]
