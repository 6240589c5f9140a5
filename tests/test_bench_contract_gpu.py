"""bench.py's one-line JSON contract (metric, whole-job value, roofline and, with --full, cpu_baseline objects) on short runs, the
plain run (the headline only, --dump-outputs) and the N > 1 launch path: two ranks on ONE device over gloo (BENCH_BACKEND=gloo) --
the only multi-rank form a 1-GPU box can run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=1200):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=timeout,
                         cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return json.loads([ln for ln in out.stdout.strip().splitlines() if ln.startswith('{')][-1])


def test_bench_json_line(dev, tmp_path):
    detail = str(tmp_path / 'detail.json')
    d = _run(['--steps', '2', '--warmup', '1', '--pairs-per-step', '4', '--keypts', '600', '--detail-json', detail, '--full'])
    assert d['metric'] == 'registration pairs/sec' and d['unit'] == 'pairs/s' and d['higher_is_better'] is True
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['warmup'] == 1 and d['scaling'] == 'weak'
    assert d['dtype'] == 'f32' and d['data'] == 'synthetic' and d['vs_baseline'] is None
    assert abs(d['value'] - 4 * 2 / (d['ms_per_step'] * 2e-3)) < 1e-6 * d['value']           # pairs / wall time
    assert 'workload' in d['config'] and 'model' not in d['config'] and 'configs[1]' in d['config']['workload']
    r = d['roofline']
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and r['peak'] == 157.3 and r['launches'] == 2
    # achieved / frac = flops of the ISSUED matrix instructions (the Winograd-domain kernel runs 0.508 of the dense count): a fraction
    # of the peak, never above 1; the dense algorithmic count over the same time rides along as dense_equivalent_tflops
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and 0.1 < r['frac'] < 1.0
    assert abs(r['useful_fraction_of_dense'] - 40 * 1024 / (9 * 140 * 64)) < 1e-12
    assert abs(r['dense_equivalent_tflops'] * r['useful_fraction_of_dense'] - r['achieved']) < 1e-9 * r['achieved']
    assert r['traffic'] is None or (r['traffic'] > 0 and 'replayed' in r['traffic_source'])
    assert 'k_cyl_net_wg' in r['kernel']
    # the opt-in split-f16 region: its own keys, the headline untouched
    rs = d['roofline_split']
    assert 'k_cyl_net_h3' in rs['kernel'] and 'f16x3 split' in rs['arithmetic'] and rs['peak'] == 2500.0 and rs['launches'] == 2
    assert abs(rs['frac'] - rs['achieved'] / rs['peak']) < 1e-9 and 0.05 < rs['frac'] < 1.0
    assert rs['error_vs_float64'] < 1e-5 and rs['error_vs_float64'] <= 1.5 * rs['error_vs_float64_fp32_kernel']
    assert abs(d['value_split'] - 4 * 2 / (d['ms_per_step_split'] * 2e-3)) < 1e-6 * d['value_split']
    assert d['split']['registered_ok'].startswith('8/8') and d['split']['max_abs_pose_difference_vs_f32_kernels'] < 1e-3
    # every kernel SURVEY 8(d) gives a roofline class: A1, A2, A4, A6, A8, A10, A11 head, A12, A13 -- compact entries
    names = ' '.join(o['kernel'] for o in d['roofline_other'])
    for k in ('k_cost_net', 'k_grid_query', 'k_vox_', 'k_vn_gather', 'k_select_patches', 'k_patch_voxelize', 'k_desc_head', 'k_nn1', 'k_fps'):
        assert k in names, k
    for o in d['roofline_other']:
        assert set(o) - {'traffic_ratio_incl_pf'} == {'kernel', 'bound', 'frac', 'avg_us', 'traffic_ratio'}
        assert o['avg_us'] > 0 and (o['frac'] is None or 0 < o['frac'] < 1.0), o
    vg = [o for o in d['roofline_other'] if o['kernel'] == 'k_vn_gather'][0]
    # the hoisted form's PF table is a deliberate round trip: its traffic is judged against algorithmic + PF bytes (close to 1), not explained away
    assert vg['traffic_ratio'] is None or 0.8 < vg['traffic_ratio_incl_pf'] < 1.6, vg
    assert d['single_pair_latency_ms'] > 0 and d['keypoint_stage_ms']['one_pair'] > 0 and d['keypoint_stage_ms']['per_step'] > 0
    l15 = d['single_pair_latency_ms_1500']               # one caller at the reference's operating point (1500 keypoints), both arithmetics
    assert set(l15) == {'f32', 'split'} and 0 < l15['split'] and 0 < l15['f32'] < 200
    c = d['cpu_baseline']
    assert c['kind'] in ('reference cores (pyramid) + restated model', 'port') and c['cores'] >= 1 and c['workers'] >= 1 and c['value'] > 0 and c['unit'] == 'pairs/s'
    assert 'nothing scaled' in c['sample'] and c['stages_s']['descriptors'] > 0
    # the oracle run of the baseline leg is also the checker of the product path on the same pair (same permutations, seed 0)
    par = c['parity']
    assert set(par) >= {'keypoints_equal', 'matches_differing', 'pose_max_abs_diff'}
    assert par['keypoints_equal'] is True and par['matches_differing'] <= max(2, par['matches'] // 200) and par['pose_max_abs_diff'] < 1e-4
    # descriptor rows beyond 1e-4 are allowed only with their cause shown: a patch point on a voxel ball surface whose fp32 decision flips
    # with the last bits of the aligned coordinates (buffer_amd/diagnose.py); every other row within round-off
    assert par['desc_rows_over_1e_4_not_explained_by_a_ball_surface_flip'] == 0 and par['desc_max_abs_diff_other_rows'] < 1e-4
    ps = c['parity_split']                                # the same pair on the split-f16 CNN kernels against the same oracle run
    assert ps['keypoints_equal'] is True and ps['matches_differing'] <= max(2, ps['matches'] // 200) and ps['pose_max_abs_diff'] < 1e-4
    assert ps['desc_rows_over_1e_4_not_explained_by_a_ball_surface_flip'] == 0
    assert d['config']['registered_ok'].startswith('8/8') and d['config']['distinct_pairs_per_gpu'] == 4      # = pairs per step
    # the driver keeps the last 2000 characters of the line: the four round-4 keys and every compact entry must be inside them
    line = json.dumps(d)
    tail = line[-2000:]
    for k in ('"single_pair_latency_ms"', '"single_pair_latency_ms_1500"', '"keypoint_stage_ms"', '"roofline_other"', 'k_grid_query', 'k_fps'):
        assert k in tail, k
    full = json.load(open(detail))
    assert full['roofline_other'][0]['launches'] > 0 and 'timed_kernel_ms_per_step' in full
    # instruction counts the vector-issue roofline is priced with come from profiles/instr.json, measured on THIS library version
    vox = [o for o in full['roofline_other'] if o['kernel'].startswith('k_patch_voxelize')][0]
    assert vox['bound'] == 'valu' and vox['instr_current'] is True, 'profiles/instr.json is stale: re-run tools/profile_round.sh (make_instr.py)'


def test_bench_plain_run_is_the_headline_and_dumps_the_last_step(dev, tmp_path):
    """Without --full: the headline keys and the dominant kernel's roofline, nothing that takes runs of its own; --dump-outputs writes
    the poses of the last timed step.  16 distinct pairs, 4 per step: the warm-up step registers pairs 0-3, the timed steps 4-7,
    8-11 and 12-15, so the dump must hold the poses of pairs 12-15 (synth.make_pair(2012 .. 2015)) in that order."""
    from buffer_amd import synth
    out = tmp_path / 'out'
    steps, warmup, pps, distinct = 3, 1, 4, 16
    d = _run(['--steps', str(steps), '--warmup', str(warmup), '--pairs-per-step', str(pps), '--distinct-pairs', str(distinct),
              '--keypts', '600', '--dump-outputs', str(out)])
    assert d['metric'] == 'registration pairs/sec' and d['unit'] == 'pairs/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['steps'] == 3 and d['warmup'] == 1 and abs(d['value'] - 4 * 3 / (d['ms_per_step'] * 3e-3)) < 1e-6 * d['value']
    assert d['roofline']['launches'] == 3 and d['config']['registered_ok'].startswith('12/12')
    for k in ('cpu_baseline', 'roofline_other', 'roofline_split', 'value_split', 'split', 'single_pair_latency_ms', 'keypoint_stage_ms'):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ['poses.npy']
    poses = np.load(out / 'poses.npy')
    assert poses.shape == (4, 4, 4) and poses.dtype == np.float32 and np.isfinite(poses).all()
    R = poses[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-3                 # rigid poses
    # each pose registers its own pair of the last step (bench.py's criterion: RTE < 0.3 m and RRE < 15 deg) and no pair of the
    # first timed step
    def ok(T, gt):
        rte = np.linalg.norm(T[:3, 3] - gt[:3, 3])
        rre = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3].T @ gt[:3, :3]) - 1) / 2, -1, 1)))
        return rte < 0.3 and rre < 15.0
    gts = {k: synth.make_pair(2000 + k)['relt_pose'] for k in range(warmup * pps, distinct)}
    last = [((warmup + steps - 1) * pps + j) % distinct for j in range(pps)]
    for j, k in enumerate(last):
        assert ok(poses[j].astype(np.float64), gts[k]), f'dumped pose {j} does not register pair {k}'
    assert not any(ok(poses[j].astype(np.float64), gts[warmup * pps + j]) for j in range(pps)), 'the dump holds the first timed step'


def test_bench_surface_workload_line(dev, tmp_path):
    """--workload surface: the drop-in mode measured -- every operator of the reference's import surface through the shim packages in
    the reference's call order (7 batch_query + 2 subsample_batch with numpy in / out, 2 FPS + 4 gathers, ball_query + grouping for the
    patches and for the 420 voxel centres, 2 KNN, svd), the same calls on the host beside them, and each shim result equal to the CPU's."""
    detail = str(tmp_path / 'surface.json')
    d = _run(['--workload', 'surface', '--keypts', '300', '--steps', '3', '--detail-json', detail])
    assert d['metric'] == 'registration pairs/sec' and d['unit'] == 'pairs/s' and d['n_gpus'] == 1 and d['vs_baseline'] is None
    assert 'drop-in mode' in d['config']['workload'] and 'NOT a registration rate' in d['config']['workload']
    s = d['surface']
    by = {o['op']: o for o in s['ops']}
    want = {'cpp_neighbors.batch_query': 7, 'cpp_subsampling.subsample_batch': 2, 'pnt2.furthest_point_sample': 2, 'pnt2.gather_operation': 4,
            'pnt2.ball_query(0.3, 512)': 2, 'pnt2.grouping_operation (patches)': 2, 'pnt2.ball_query(0.267, 10)': 2,
            'pnt2.grouping_operation (voxels)': 2, 'knn_cuda.KNN(k=1)': 2, 'torch_batch_svd.svd': 2, 'pnt2.three_nn': 2}
    assert {k: v['calls'] for k, v in by.items()} == want
    for o in s['ops']:
        assert set(o) == {'op', 'site', 'calls', 'ms_gpu', 'ms_cpu', 'equal_to_cpu', 'shapes'}
        assert o['ms_gpu'] > 0 and o['ms_cpu'] > 0 and o['equal_to_cpu'] is True, o
    on_path = [o for o in s['ops'] if 'svd' not in o['op'] and 'three_nn' not in o['op']]
    assert abs(s['sum_ms_gpu'] - sum(o['ms_gpu'] for o in on_path)) < 0.01 and abs(d['value'] - 1e3 / s['sum_ms_gpu']) < 1e-3 * d['value']
    assert abs(s['sum_ms_cpu'] - sum(o['ms_cpu'] for o in on_path)) < 0.5
    assert len(s['fused']) == 5 and all(f['ms'] > 0 and f['replaces'] for f in s['fused']) and s['buffer_pipeline_whole_pair_ms'] > 0
    c = d['cpu_baseline']
    assert c['cores'] == 1 and c['unit'] == 'pairs/s' and abs(c['value'] - 1e3 / s['sum_ms_cpu']) < 1e-2 * c['value']
    full = json.load(open(detail))
    assert len(full['calls']) == 29 and all(x['equal'] for x in full['calls'])


def test_bench_strong_scaling_mode_two_ranks_over_gloo(dev):
    """--total-pairs: the job's pairs of a step are fixed and dealt i -> rank i mod N (5 pairs on 2 ranks: 3 + 2)."""
    d = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--total-pairs', '5', '--keypts', '400', '--no-cpu-baseline', '--no-split', '--full'],
             env={'BENCH_BACKEND': 'gloo'})
    assert d['n_gpus'] == 2 and d['scaling'] == 'strong' and d['config']['pairs_per_step_job'] == 5
    assert abs(d['value'] - 2 * 5 / (d['ms_per_step'] * 2e-3)) < 1e-6 * d['value']
    assert d['config']['gathered_poses'] == [6, 6] and d['config']['registered_ok'].startswith('6/6')      # rank 0: 3 pairs x 2 steps


def test_bench_two_ranks_on_one_device_over_gloo(dev):
    """`python bench.py --gpus 2` with no launcher: bench.py starts torch.distributed.run itself; both ranks share cuda:0."""
    d = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--pairs-per-step', '3', '--keypts', '400', '--no-cpu-baseline', '--no-split', '--full'],
             env={'BENCH_BACKEND': 'gloo'})
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and 'cpu_baseline' not in d
    assert d['config']['parallelism'] == 'pair-sharded x2' and d['config']['gathered_poses'] == [6, 6]     # steps x pairs, per rank
    # first-contact diagnostics: every rank's own clock, host share, set-up time, dominant-kernel time and core share
    pr = d['config']['per_rank']
    assert [r['rank'] for r in pr] == [0, 1]
    for r in pr:
        assert set(r) == {'rank', 'elapsed_s', 'host_busy_frac', 'setup_s', 'main_kernel_ms', 'pinned_cpus', 'numa_node'}
        assert 0 < r['elapsed_s'] <= d['ms_per_step'] * 2e-3 + 1e-3 and 0 <= r['host_busy_frac'] <= 1.5 and r['main_kernel_ms'] > 0
        assert r['pinned_cpus'] >= 1                       # two ranks on one node: each pinned to its own share of the cores
    assert abs(max(r['elapsed_s'] for r in pr) - d['ms_per_step'] * 2e-3) < 1e-3
    assert abs(d['value'] - 2 * 2 * 3 / (d['ms_per_step'] * 2e-3)) < 1e-6 * d['value']                      # whole-job pairs / max-rank time
    assert d['config']['registered_ok'].startswith('6/6')


def test_bench_refuses_a_world_size_mismatch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], capture_output=True, text=True, cwd=ROOT,
                         env=dict(os.environ, WORLD_SIZE='1', RANK='0'), timeout=300)
    assert out.returncode != 0 and 'torch.distributed.run' in (out.stderr + out.stdout)


def test_bench_kitti_and_stream_workloads(dev):
    k = _run(['--workload', 'kitti', '--steps', '1', '--warmup', '1', '--pairs-per-step', '2', '--keypts', '300', '--no-cpu-baseline',
              '--distinct-pairs', '2', '--full'])
    assert 'configs[3]' in k['config']['workload'] and k['value'] > 0 and k['config']['sds_points'][0] > 3000
    s = _run(['--workload', 'stream', '--stream-pairs', '24', '--pairs-per-step', '8', '--keypts', '600'])
    assert 'configs[2]' in s['config']['workload'] and s['quality']['pairs'] == 24 and len(s['quality']['per_scene']) == 8
    assert s['quality']['dgr_recall'] >= 0.8 and s['value'] > 0


def test_stream_two_ranks_score_every_pair_and_equal_one_rank(dev):
    """--workload stream at N = 2 (two ranks on one device over gloo): rank 0 scores ALL gathered poses, and Registration
    Recall / DGR recall / per-pair errors equal the one-rank run of the same stream."""
    args = ['--workload', 'stream', '--stream-pairs', '24', '--pairs-per-step', '6', '--keypts', '600']
    one = _run(args)
    two = _run(['--gpus', '2'] + args, env={'BENCH_BACKEND': 'gloo'})
    assert two['n_gpus'] == 2 and two['scaling'] == 'strong' and 'all ranks' in two['quality']['scored']
    q1, q2 = one['quality'], two['quality']
    assert q2['pairs'] == 24 and q1['pairs'] == 24
    assert q1['registration_recall'] == q2['registration_recall'] and q1['dgr_recall'] == q2['dgr_recall']
    assert q1['per_scene'] == q2['per_scene']


def test_rccl_collectives_of_the_multi_gpu_path_run_on_this_box(dev):
    """The collectives bench.py / dist.py issue at N > 1 (backend 'nccl' = RCCL: barrier, all_gather of f32 poses, all_reduce MAX
    of an f64 time, broadcast of int64 limits) on a world of ONE rank over the real RCCL backend -- what a 1-GPU box can check
    of the RCCL side; rank arithmetic and gathers are covered over gloo with two ranks."""
    code = '''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from buffer_amd import dist as bd
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
dev = torch.device("cuda", 0); torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=dev)
dist.barrier()
mine = torch.eye(4, device=dev).repeat(5, 1, 1)
out = [torch.empty_like(mine)]
dist.all_gather(out, mine)
assert torch.equal(out[0], mine)
t = torch.tensor([1.25], dtype=torch.float64, device=dev)
dist.all_reduce(t, op=dist.ReduceOp.MAX)
assert t.item() == 1.25
assert bd.broadcast_limits([17, 20, 24], device=dev) == [17, 20, 24]
allp = bd.gather_poses([0, 1, 2], torch.eye(4, device=dev).repeat(3, 1, 1) * 2, 3, device=dev)
assert allp.shape == (3, 4, 4) and float(allp[2, 0, 0]) == 2.0
dist.destroy_process_group()
print("rccl ok")
''' % ROOT
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and 'rccl ok' in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
