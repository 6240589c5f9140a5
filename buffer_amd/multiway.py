"""Multiway registration of 3DMatch-layout scenes: register a scene's pairs through the device pipeline, weight every pair by its
information matrix, and place all fragments in one frame by a pose graph with line processes (buffer_amd/posegraph.py; the optimiser
is csrc/posegraph.hip, all scenes in one call per pass).

    python -m buffer_amd.multiway --root R [--dataset 3DMatch|3DLoMatch] [--scenes S ...] [--all-pairs] [--min-overlap 0.3]
                                  [--preference 1.0] [--prune 0.25] [--log-root L] [--log-name N] [--preset P] [--batch B] [--limits a,b,c]

Per scene: the pairs of gt.log (or, with --all-pairs, every i < j whose overlap under the ESTIMATED pose is at least --min-overlap)
-> driver.register_pairs -> posegraph.scene_edges on the fragments voxelised at the configuration's `downsample` (radius 1.5 voxel,
all edges uncertain) -> posegraph.optimize_two_pass -> <L>/<scene>/multiway_trajectory.log (fragment -> world, fragment 0 fixed) and
<L>/<scene>/<log-name>: the driver's pair log rewritten from the optimised poses.  Prints one JSON line."""
import json
import os
import time

import numpy as np

from . import driver, evaluate, pairs as bpairs, posegraph
from .plyio import load_gt_log, read_ply
from .threedmatch import DGR_THRESHOLDS, SCENES


class ScenePairSet(driver.PairTestSet):
    """pairs (scene, i, j) of 3DMatch-layout scenes for driver.register_pairs: source fragment i, target fragment j; gt: per pair the
    pose source -> target, or None where it is not known (the identity then stands in: it only feeds metrics nobody asks for here)"""

    def __init__(self, root, items, gt, cfg):
        self.root = os.path.join(root, 'test', '3DMatch', 'fragments')
        self.files, self.gt = list(items), list(gt)
        self.downsample, self.voxel_size_0, self.max_num_pts = cfg.downsample, cfg.voxel_size_0, cfg.max_num_pts

    def raw_pair(self, index):
        scene, i, j = self.files[index]
        return tuple(read_ply(os.path.join(self.root, scene, f'cloud_bin_{k}.ply')) for k in (i, j))

    def meta(self, index, device=None):
        scene, i, j = self.files[index]
        return {'src_id': f'{scene}/cloud_bin_{i}', 'tgt_id': f'{scene}/cloud_bin_{j}',
                'relt_pose': np.eye(4) if self.gt[index] is None else self.gt[index]}


def _count_fragments(frag_dir):
    n = 0
    while os.path.exists(os.path.join(frag_dir, f'cloud_bin_{n}.ply')):
        n += 1
    return n


def _registration_recall(gt_dir, n, pair_ids, poses):
    """the scene's Registration Recall of pair poses (source i -> target j) against gt.log / gt.info; None without them or without a
    non-consecutive ground-truth pair"""
    if not (os.path.exists(os.path.join(gt_dir, 'gt.log')) and os.path.exists(os.path.join(gt_dir, 'gt.info'))) or not pair_ids:
        return None
    gt_pairs, gt_traj = evaluate.read_trajectory(os.path.join(gt_dir, 'gt.log'))
    n_frag, gt_info = evaluate.read_trajectory_info(os.path.join(gt_dir, 'gt.info'))
    if not any(int(p[1]) - int(p[0]) > 1 for p in gt_pairs):
        return None
    est_pairs = np.array([[str(i), str(j), str(n)] for i, j in pair_ids])
    est = np.array([np.linalg.inv(np.asarray(p, np.float64)) for p in poses]).astype(np.float32)      # the log holds the inverse
    return float(evaluate.evaluate_registration(n_frag, est, est_pairs, gt_pairs, gt_traj, gt_info)[1])


def _mean(xs):
    xs = [x for x in xs if x is not None]
    return float(np.mean(xs)) if xs else None


def main(argv=None, override_poses=None):
    """python -m buffer_amd.multiway --root <data root> ...  (one process, one GPU).  override_poses: {(scene, i, j): 4x4} replaces
    the registered pose of those pairs before the graph is built (experiments and tests: what does a wrong pair do?).
    Returns dict(scene -> dict(poses f64[n,4,4], edges, dropped, pruned, result))."""
    import argparse

    import torch

    from .config import DRIVER_PRESETS, preset
    from .pipeline import BufferPipeline
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument('--root', required=True)
    ap.add_argument('--dataset', default='3DMatch', choices=['3DMatch', '3DLoMatch'])
    ap.add_argument('--scenes', nargs='+', default=None, help='default: the eight test scenes')
    ap.add_argument('--all-pairs', action='store_true', help='every i < j instead of the pairs of gt.log; kept by estimated overlap')
    ap.add_argument('--min-overlap', type=float, default=0.3, help='with --all-pairs: least overlap under the estimated pose')
    ap.add_argument('--preference', type=float, default=1.0, help='line-process weight = preference * radius^2 * mean matched count')
    ap.add_argument('--prune', type=float, default=0.25, help='edges whose line-process weight falls below this are removed')
    ap.add_argument('--no-optimize', action='store_true', help='stop after the edges are built (what the optimisation step costs)')
    ap.add_argument('--log-root', default=None)
    ap.add_argument('--log-name', default=time.strftime('%m%d%H%M') + '_multiway.log')
    ap.add_argument('--preset', default=DRIVER_PRESETS['threedmatch'][0])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--limits', default=None, help='frozen neighbourhood limits "a,b,c" (default: calibrated on the first pairs)')
    a = ap.parse_args(argv)
    try:
        cfg = preset(a.preset, 'threedmatch')
    except ValueError as e:
        ap.error(str(e))
    scenes = list(SCENES if a.scenes is None else a.scenes)
    log_root = a.log_root or f'log_{a.dataset}_multiway'
    override_poses = override_poses or {}
    _, _, dev, _ = driver.init()

    frag_root = os.path.join(a.root, 'test', '3DMatch', 'fragments')
    gt_dirs = {s: os.path.join(a.root, 'test', '3DMatch', 'gt_result', s) if a.dataset == '3DMatch' else os.path.join(a.root, 'test', a.dataset, s)
               for s in scenes}
    items, gts, n_of, world = [], [], {}, {}
    for s in scenes:
        n = n_of[s] = _count_fragments(os.path.join(frag_root, s))
        if n == 0:
            ap.error(f'no cloud_bin_0.ply under {os.path.join(frag_root, s)}')
        try:
            world[s] = np.array(bpairs.read_poses(None, n, os.path.join(frag_root, s)))
        except FileNotFoundError:
            world[s] = None
        log = load_gt_log(gt_dirs[s]) if os.path.exists(os.path.join(gt_dirs[s], 'gt.log')) else {}
        if a.all_pairs:
            ids = [(i, j) for i in range(n) for j in range(i + 1, n)]
        else:
            if not log:
                ap.error(f'{gt_dirs[s]}/gt.log is missing (--all-pairs registers every pair instead)')
            ids = [tuple(int(x) for x in k.split('_')) for k in log]
        for i, j in ids:
            items.append((s, i, j))
            if f'{i}_{j}' in log:
                gts.append(np.linalg.inv(log[f'{i}_{j}']))                              # gt.log holds j -> i
            elif world[s] is not None:
                gts.append(np.linalg.inv(world[s][j]) @ world[s][i])
            else:
                gts.append(None)
    ds = ScenePairSet(a.root, items, gts, cfg)

    t0 = time.perf_counter()
    pipe = BufferPipeline(cfg, dev)
    if a.limits:
        pipe.limits = [int(x) for x in a.limits.split(',')]
    else:
        host = []
        for k in range(min(len(ds), 8)):
            smp = ds.item(k, dev)
            host.append({key: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for key, v in smp.items()})
        pipe.calibrate(host)
    direct = driver.register_pairs(pipe, ds, range(len(ds)), a.batch).cpu().numpy().astype(np.float64)
    for k, it in enumerate(items):
        if it in override_poses:
            direct[k] = np.asarray(override_poses[it], np.float64)
    t_reg = time.perf_counter() - t0

    t0 = time.perf_counter()
    radius = 1.5 * cfg.downsample
    per, graphs = {}, []
    for s in scenes:
        idx = [k for k, it in enumerate(items) if it[0] == s]
        ids = [items[k][1:] for k in idx]
        clouds = bpairs.downsample_clouds([read_ply(os.path.join(frag_root, s, f'cloud_bin_{k}.ply'), drop_non_finite=True) for k in range(n_of[s])],
                                          cfg.downsample, dev)
        keep = list(range(len(ids)))
        if a.all_pairs and ids:
            st = bpairs.pair_statistics(clouds, ids, np.array([posegraph.project_rigid(direct[k]) for k in idx]), radius, symmetric=True)
            ov = np.minimum(st['overlap'], st['reverse']['overlap'])
            keep = [k for k in keep if ov[k] >= a.min_overlap]
        edges, dropped = posegraph.scene_edges(clouds, [ids[k] for k in keep], direct[[idx[k] for k in keep]], radius)
        for e in edges + dropped:
            e['index'] = keep[e['index']]                                               # position in the scene's pair list
        init, lost = posegraph.initial_poses(n_of[s], edges, fixed=0)
        per[s] = dict(idx=idx, ids=ids, edges=edges, dropped=dropped, not_overlapping=[ids[k] for k in range(len(ids)) if k not in set(keep)],
                      lost=lost)
        graphs.append(dict(n=n_of[s], edges=edges, init=init, fixed=0, mu=posegraph.line_process_weight(edges, radius, a.preference)))
    t_edges = time.perf_counter() - t0

    t0 = time.perf_counter()
    results = [None] * len(scenes) if a.no_optimize else posegraph.optimize_two_pass(graphs, threshold=a.prune, device=dev)
    t_opt = time.perf_counter() - t0

    out_scenes, ret = {}, {}
    rr_direct, rr_opt, ok_direct, ok_opt, rmse = [], [], [], [], []
    for s, g, res in zip(scenes, graphs, results):
        p = per[s]
        W = g['init'] if res is None else res['poses']
        back = direct[p['idx']].copy() if p['idx'] else np.zeros((0, 4, 4))
        for k, (i, j) in enumerate(p['ids']):
            if i not in p['lost'] and j not in p['lost']:
                back[k] = posegraph.rigid_inverse(W[j]) @ W[i]                          # source i -> target j; the log holds T_ij = its inverse
        posegraph.write_trajectory(os.path.join(log_root, s, 'multiway_trajectory.log'), W)
        log = os.path.join(log_root, s, a.log_name)
        if os.path.exists(log):
            os.remove(log)
        for (i, j), T in zip(p['ids'], back):
            evaluate.append_log(log, i, j, T)
        rr_direct.append(_registration_recall(gt_dirs[s], n_of[s], p['ids'], direct[p['idx']]))
        rr_opt.append(_registration_recall(gt_dirs[s], n_of[s], p['ids'], back))
        for k, gi in enumerate(p['idx']):
            if gts[gi] is not None:
                ok_direct.append(evaluate.dgr_success(direct[gi], gts[gi], *DGR_THRESHOLDS)[0])
                ok_opt.append(evaluate.dgr_success(back[k], gts[gi], *DGR_THRESHOLDS)[0])
        pruned = [] if res is None else [(e['i'], e['j']) for e, m in zip(p['edges'], res['pruned']) if m]
        row = dict(nodes=n_of[s], edges=len(p['edges']), dropped=[(d['i'], d['j']) for d in p['dropped']], pruned=pruned,
                   not_overlapping=p['not_overlapping'], disconnected=p['lost'],
                   solves=None if res is None else [res['first']['solves'], res['solves']],
                   status=None if res is None else [res['first']['status'], res['status']])
        if world[s] is not None:
            err = posegraph.trajectory_error(W, world[s], fixed=0)
            row['trajectory_rmse'] = dict(rte=err['rte_rmse'], rre=err['rre_rmse'])
            rmse.append(err['rte_rmse'])
        out_scenes[s] = row
        ret[s] = dict(poses=W, edges=p['edges'], dropped=p['dropped'], pruned=pruned, result=res, pair_ids=p['ids'], pair_poses=back,
                      direct_poses=direct[p['idx']])
    out = dict(dataset=a.dataset, preset=a.preset, pairs=len(items), limits=pipe.limits, log_name=a.log_name, scenes=out_scenes,
               direct=dict(registration_recall=_mean(rr_direct), dgr_recall=float(np.mean(ok_direct)) if ok_direct else None),
               optimized=dict(registration_recall=_mean(rr_opt), dgr_recall=float(np.mean(ok_opt)) if ok_opt else None),
               trajectory_rmse=_mean(rmse), seconds=dict(register=t_reg, edges=t_edges, optimize=t_opt))
    print(json.dumps(out))
    return ret


if __name__ == '__main__':
    main()
