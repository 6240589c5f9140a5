"""Per-stage ground-truth metrics, the parts that need no device: the C ABI of buf_match_metrics (argument checks come before any
device call), evaluate.stage_summary on hand-written count rows, the --stage-metrics option of the three drivers and the
count gather over two gloo ranks."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from buffer_amd import _lib, build
    build.build()
    return _lib.lib()


def _call(lib, npairs=2, P=100, tau_kp=0.1, tau_match=0.1, dist_th=0.1, null=None):
    """buf_match_metrics with placeholder device pointers: only argument checks may run (they precede any device call)."""
    fake, nul = C.c_void_p(0x1000), C.c_void_p(0)
    ptr = {k: (nul if k == null else fake) for k in ('kp', 's_nn', 't_nn', 'T_gt', 'T_est', 'counts')}
    rc = lib.buf_match_metrics(ptr['kp'], ptr['s_nn'], ptr['t_nn'], npairs, P, ptr['T_gt'], ptr['T_est'], tau_kp, tau_match, dist_th,
                               ptr['counts'], nul, nul)
    return rc, lib.buf_last_error().decode()


def test_match_metrics_is_exported_and_bound(lib):
    from buffer_amd import _lib, ops
    assert "buf_match_metrics" in _lib.exported_symbols()
    assert lib.buf_match_metrics.argtypes is not None and len(lib.buf_match_metrics.argtypes) == 13
    assert len(ops.METRIC_COLUMNS) == 7
    header = open(os.path.join(ROOT, 'include', 'buffer_hip.h')).read()
    assert re.search(r'#define\s+BUF_METRICS_NCOUNT\s+7\b', header)
    for i, name in enumerate(ops.METRIC_COLUMNS):                    # the Python column order is the header's
        assert re.search(rf'#define\s+BUF_METRICS_{name.upper()}\s+{i}\b', header), name


@pytest.mark.parametrize("npairs,P", [(-1, 100), (2, -1), (-3, -3)])
def test_match_metrics_rejects_negative_sizes(lib, npairs, P):
    rc, msg = _call(lib, npairs=npairs, P=P)
    assert rc == -1 and "npairs" in msg


@pytest.mark.parametrize("which", ["tau_kp", "tau_match", "dist_th"])
@pytest.mark.parametrize("value", [0.0, -0.1, math.nan, math.inf, -math.inf])
def test_match_metrics_rejects_a_bad_threshold(lib, which, value):
    rc, msg = _call(lib, **{which: value})
    assert rc == -1 and which in msg


@pytest.mark.parametrize("null", ["kp", "s_nn", "t_nn", "T_gt", "T_est", "counts"])
def test_match_metrics_rejects_a_null_pointer(lib, null):
    rc, msg = _call(lib, null=null)
    assert rc == -1 and "null" in msg


def test_match_metrics_empty_call_succeeds_and_touches_nothing(lib):
    for null in (None, "kp", "counts"):                               # nothing is dereferenced: null pointers are fine here
        assert _call(lib, npairs=0, P=100, null=null)[0] == 0
        assert _call(lib, npairs=4, P=0, null=null)[0] == 0
        assert _call(lib, npairs=0, P=0, null=null)[0] == 0
    assert _call(lib, npairs=0, tau_kp=-1.0)[0] == -1                 # a bad threshold is refused whatever the size


def test_match_metrics_python_checks_shapes():
    torch = pytest.importorskip("torch")
    from buffer_amd import _lib, ops
    with pytest.raises(_lib.BufferHipError):                          # host tensors: there is no CPU path
        ops.match_metrics(torch.zeros(8, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32),
                          np.eye(4)[None], torch.eye(4)[None], 0.1, 0.1, 0.1)


# ---------------------------------------------------------------------------------------------------- stage_summary
#                rep_src rep_tgt nn_inl mutual mutual_inl cons cons_true        (P = 100)
ROWS = np.array([[80, 60, 50, 40, 30, 20, 10],
                 [20, 40, 5, 10, 5, 4, 4],           # nn_inl / P = 0.05: NOT above the FMR ratio (strict)
                 [0, 0, 6, 0, 0, 0, 0],             # no mutual match, empty consensus set: those ratios count as 0
                 [-1, -1, -1, -1, -1, -1, -1]])      # not evaluated


def test_stage_summary_ratios():
    from buffer_amd import evaluate
    s = evaluate.stage_summary(ROWS, 100)
    assert s['pairs'] == 3 and s['not_evaluated'] == 1
    assert s['repeatability'] == pytest.approx((0.7 + 0.3 + 0.0) / 3, abs=1e-15)
    assert s['inlier_ratio'] == pytest.approx((0.5 + 0.05 + 0.06) / 3, abs=1e-15)
    assert s['mutual_inlier_ratio'] == pytest.approx((0.75 + 0.5 + 0.0) / 3, abs=1e-15)
    assert s['consensus_precision'] == pytest.approx((0.5 + 1.0 + 0.0) / 3, abs=1e-15)
    assert s['fmr'] == pytest.approx(2 / 3, abs=1e-15)                 # 0.5 and 0.06 are above 0.05, 0.05 itself is not
    assert set(s) == {'pairs', 'not_evaluated', 'repeatability', 'inlier_ratio', 'fmr', 'mutual_inlier_ratio', 'consensus_precision'}


def test_stage_summary_fmr_ratio_is_a_parameter():
    from buffer_amd import evaluate
    assert evaluate.stage_summary(ROWS, 100, fmr_ratio=0.04)['fmr'] == 1.0
    assert evaluate.stage_summary(ROWS, 100, fmr_ratio=0.055)['fmr'] == pytest.approx(2 / 3, abs=1e-15)
    assert evaluate.stage_summary(ROWS, 100, fmr_ratio=0.06)['fmr'] == pytest.approx(1 / 3, abs=1e-15)
    assert evaluate.stage_summary(ROWS, 100, fmr_ratio=0.5)['fmr'] == 0.0


def test_stage_summary_without_evaluated_pairs():
    from buffer_amd import evaluate
    for rows in (ROWS[3:], np.zeros((0, 7), np.int32)):
        s = evaluate.stage_summary(rows, 100)
        assert s['pairs'] == 0 and s['not_evaluated'] == len(rows)
        assert all(s[k] == 0.0 for k in ('repeatability', 'inlier_ratio', 'fmr', 'mutual_inlier_ratio', 'consensus_precision'))
    assert evaluate.stage_summary(ROWS[:1], 0)['inlier_ratio'] == 0.0   # P = 0: a zero denominator as well


def test_stage_report_per_scene_adds_up_and_json_roundtrip(tmp_path):
    import json
    from buffer_amd import evaluate, threedmatch
    scenes = ['a', 'a', 'b', 'b']
    rep = threedmatch.stage_report(scenes, ROWS, 100)
    assert list(rep['per_scene']) == ['a', 'b']
    assert rep['per_scene']['b']['pairs'] == 1 and rep['per_scene']['b']['not_evaluated'] == 1
    n = sum(v['pairs'] for v in rep['per_scene'].values())
    assert n == rep['pairs'] and sum(v['not_evaluated'] for v in rep['per_scene'].values()) == rep['not_evaluated']
    for k in ('repeatability', 'inlier_ratio', 'fmr', 'mutual_inlier_ratio', 'consensus_precision'):
        assert sum(v[k] * v['pairs'] for v in rep['per_scene'].values()) / n == pytest.approx(rep[k], abs=1e-12)
    path = str(tmp_path / 'logs' / 'stage_metrics.json')
    evaluate.write_stage_metrics(path, ['p0', 'p1', 'p2', 'p3'], ROWS, 100, rep)
    back = json.load(open(path))
    assert back['columns'] == list(evaluate.STAGE_COLUMNS) and back['num_keypts'] == 100
    assert [p['id'] for p in back['pairs']] == ['p0', 'p1', 'p2', 'p3']
    assert np.array_equal(np.array([p['counts'] for p in back['pairs']]), ROWS)
    assert back['summary'] == json.loads(json.dumps(rep))


def test_stage_columns_agree():
    from buffer_amd import evaluate, ops
    assert tuple(evaluate.STAGE_COLUMNS) == tuple(ops.METRIC_COLUMNS)


# ---------------------------------------------------------------------------------------------------- drivers
# parse_args defaults of the parent commit: --stage-metrics must leave every one of them as it is
PARENT_DEFAULTS = {
    'threedmatch': dict(root='r', preset='3DMatch', dataset='3DMatch', log_root=None, batch=32, limits=None),
    'kitti': dict(root='r', preset='KITTI', batch=4, limits=None, allow_odometry_gt=False, refine_gt=False, batch_icp=16),
    'eth': dict(root='r', preset='3DMatch->ETH', scenes=None, batch=8, limits=None),
}


@pytest.mark.parametrize("name", ['threedmatch', 'kitti', 'eth'])
def test_stage_metrics_option_parses_and_is_off_by_default(name):
    import importlib
    mod = importlib.import_module(f'buffer_amd.{name}')
    a, cfg = mod.parse_args(['--root', 'r'])
    assert a.stage_metrics is False
    for k, v in PARENT_DEFAULTS[name].items():
        assert getattr(a, k) == v, (k, getattr(a, k))
    b, cfg_b = mod.parse_args(['--root', 'r', '--stage-metrics'])
    assert b.stage_metrics is True and cfg_b == cfg
    for k, v in PARENT_DEFAULTS[name].items():
        assert getattr(b, k) == v, (k, getattr(b, k))
    c, _ = mod.parse_args(['--root', 'r', '--stage-metrics', '--log-root', 'somewhere'])
    assert c.log_root == 'somewhere'


def test_register_pairs_take_the_flag():
    import inspect
    from buffer_amd import eth, kitti, threedmatch
    for fn, batch in ((threedmatch.register_pairs, 32), (kitti.register_pairs, 4), (eth.register_pairs, 32)):
        assert inspect.signature(fn).parameters['stage_metrics'].default is False
        assert inspect.signature(fn).parameters['batch'].default == batch


# ---------------------------------------------------------------------------------------------------- gather over gloo
_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from buffer_amd import dist as bd
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
rank, world = dist.get_rank(), dist.get_world_size()
def row(i):
    return [-1] * 7 if i == 3 else [1000 * i + c for c in range(7)]          # pair 3: not evaluated
for n in (7, 2, 1, 0):                                                           # odd count, one pair per rank, an empty shard, nothing
    ids = bd.shard_indices(n, rank, world)
    local = torch.tensor([row(i) for i in ids], dtype=torch.int32).reshape(-1, 7)
    allc = bd.gather_counts(ids, local, n)
    assert allc.dtype == torch.int32 and tuple(allc.shape) == (n, 7), (allc.dtype, allc.shape)
    assert allc.tolist() == [row(i) for i in range(n)], (rank, n, allc.tolist())
try:
    bd.gather_counts([5], torch.zeros(1, 7, dtype=torch.int32), 7)
    raise SystemExit('ids that break the sharding rule were accepted')
except ValueError:
    pass
try:
    bd.gather_counts(bd.shard_indices(7, rank, world), torch.zeros(1, 7, dtype=torch.int32), 7)
    raise SystemExit('a count block of the wrong height was accepted')
except ValueError:
    pass
dist.destroy_process_group()
print('ok', rank)
'''


def test_gather_counts_two_gloo_ranks(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"ok {r}" in o


def test_gather_counts_single_process():
    torch = pytest.importorskip("torch")
    from buffer_amd import dist as bd
    local = torch.arange(21, dtype=torch.int32).reshape(3, 7)
    assert torch.equal(bd.gather_counts([0, 1, 2], local, 3), local)
    assert tuple(bd.gather_counts([], torch.zeros(0, 7, dtype=torch.int32), 0).shape) == (0, 7)
