"""What the three test-set drivers (threedmatch.py, kitti.py, eth.py) and the synthetic stream (stream.py) share: raw clouds -> sample
dicts -> pipeline inputs, the chunked registration loop, the DGR summary, the common command line and the body of main().
Host code only; a data-set module keeps its file layout, its ground truth and its own scoring."""
import json
import os
import time

import numpy as np
import torch

from . import evaluate, preprocess


# ---------------------------------------------------------------------------------------------------- raw clouds -> samples
# `consts` below: any object with downsample, voxel_size_0 and max_num_pts (a test set or a Config)
def pack_pair(raws, seeds, meta, consts):
    """One pair: the two raw clouds (f32[n,3] device tensors, src then tgt), each through one preprocess.prepare_fragment call
    (two voxel levels, shuffle keyed by its seed, normals) -> the reference's sample dict of DEVICE tensors: meta +
    {src,tgt}_fds_pts, {src,tgt}_sds_pts.  `raws` may be lazy: a cloud is taken when its turn comes."""
    out = dict(meta)
    for side, raw, seed in zip(('src', 'tgt'), raws, seeds):
        it = preprocess.prepare_fragment(raw, consts.downsample, consts.voxel_size_0, consts.max_num_pts, seed=seed,
                                         denoise=getattr(consts, 'denoise', None))
        out[f'{side}_fds_pts'], out[f'{side}_sds_pts'] = it['fds_pts'], it['sds_pts']
        _log_denoise(consts, [it])
    return out


def _log_denoise(consts, fragments):
    """the removed fractions of denoised fragments -> consts.denoise_log, where the driver keeps one (run)"""
    log = getattr(consts, 'denoise_log', None)
    if log is not None:
        log.extend(f['denoise_removed'] for f in fragments if 'denoise_removed' in f)


def pack_pairs(raws, seeds, metas, consts):
    """pack_pair for B pairs with the normals of all 2B clouds estimated in ONE stacked pass (preprocess.prepare_fragments); pair by
    pair the result is that of pack_pair.  raws, seeds: 2B entries (src, tgt of pair 0, src, tgt of pair 1, ...); metas: B dicts,
    read AFTER the stacked pass is queued (a generator keeps the work of making them behind it)."""
    frs = preprocess.prepare_fragments(raws, consts.downsample, consts.voxel_size_0, consts.max_num_pts, seeds,
                                       denoise=getattr(consts, 'denoise', None))
    _log_denoise(consts, frs)
    out = []
    for k, meta in enumerate(metas):
        s = dict(meta)
        s.update(src_fds_pts=frs[2 * k]['fds_pts'], src_sds_pts=frs[2 * k]['sds_pts'],
                 tgt_fds_pts=frs[2 * k + 1]['fds_pts'], tgt_sds_pts=frs[2 * k + 1]['sds_pts'])
        out.append(s)
    return out


class PairTestSet:
    """Base of the test sets.  A subclass supplies `files` (one entry per pair), raw_pair(index) -> the two clouds as read from disk
    (f32[n,3] numpy), meta(index, device) -> dict(src_id, tgt_id, relt_pose f64[4,4] source -> target) and the voxel constants
    downsample, voxel_size_0, max_num_pts."""

    def __len__(self):
        return len(self.files)

    def item(self, index, device, seed=None):
        """The test branch of the reference's Dataset.__getitem__ on the device -> pack_pair's sample dict.  The two clouds shuffle
        with seeds 2 * index and 2 * index + 1, or both with `seed`."""
        meta = self.meta(index, device)               # before any pre-processing launch (KITTI may refine its ground truth here)
        raws = (torch.from_numpy(raw).to(device) for raw in self.raw_pair(index))
        return pack_pair(raws, (2 * index, 2 * index + 1) if seed is None else (seed, seed), meta, self)


def items_batched(dataset, indices, device):
    """dataset.item(i, device) for several pairs through pack_pairs; pair by pair the result is that of item()."""
    idx = list(indices)
    raws = [torch.from_numpy(raw).to(device) for i in idx for raw in dataset.raw_pair(i)]
    return pack_pairs(raws, [2 * i + j for i in idx for j in range(2)], (dataset.meta(i, device) for i in idx), dataset)


def upload(sample):
    """sample dict of device tensors (pack_pair) -> the inputs BufferPipeline.register takes
    (the device-side twin of pyramid.stack_sample)."""
    src, tgt = sample['src_sds_pts'], sample['tgt_sds_pts']
    return dict(points=torch.cat([src[:, :3], tgt[:, :3]]).contiguous(), features=torch.cat([src[:, 3:], tgt[:, 3:]]).contiguous(),
                lengths=np.array([src.shape[0], tgt.shape[0]], np.int32), src_raw=sample['src_fds_pts'], tgt_raw=sample['tgt_fds_pts'])


# ---------------------------------------------------------------------------------------------------- registration
def register_chunks(pipe, chunks, make, gt_of=None, refine=None):
    """Chunks of pairs through the device pipeline -> f32[k,4,4] (device) in chunk order.  chunks: lists of pair ids, which also seed
    the pipeline; make(chunk) -> the chunk's sample dicts.  The chunks are software-pipelined over two HIP streams: making chunk
    i+1 (reading, pre-processing) and its keypoint stage run beside the CNN kernels of chunk i (BufferPipeline.register_batches;
    results equal batch-by-batch calls).
    gt_of(chunk) -> the chunk's ground-truth poses: also the per-stage metric rows (register_batches, metrics_gt=: the ground truth
    is read when the chunk's clouds are, one metric launch per chunk after its pose recovery) -> (poses, counts int32[k,7]).
    refine: BufferPipeline.refine_batch's keyword arguments: every chunk's poses are also refined by dense ICP after its pose
    recovery -> one more last element, dict(poses f32[k,4,4], fitness f64[k], inlier_rmse f64[k], iterations int32[k]) (device);
    what comes before it is what a call without refine returns, bit for bit."""
    dev = pipe.device
    makers = [(lambda ch=ch: [upload(s) for s in make(ch)]) for ch in chunks]
    gts = None if gt_of is None else [(lambda ch=ch: gt_of(ch)) for ch in chunks]
    if refine is None:
        return _unrefined(dev, pipe.register_batches(makers, seeds=chunks, metrics_gt=gts), gt_of)
    out = pipe.register_batches(makers, seeds=chunks, metrics_gt=gts, refine=refine)
    refs = [o[1] for o in out] or [pipe.refine_batch([], [], **refine)]
    refined = {k: torch.cat([r[k] for r in refs]) for k in refs[0]}
    res = _unrefined(dev, [o[0] for o in out], gt_of)
    return (res if gt_of is not None else (res,)) + (refined,)


def _unrefined(dev, out, gt_of):
    """register_batches' entries -> register_chunks' result without refine"""
    poses = [p for o in out for p in (o if gt_of is None else o[0])]
    poses = torch.stack(poses) if poses else torch.zeros((0, 4, 4), dtype=torch.float32, device=dev)
    if gt_of is None:
        return poses
    counts = torch.cat([o[1] for o in out]) if out else torch.zeros((0, 7), dtype=torch.int32, device=dev)
    return poses, counts


def register_pairs(pipe, dataset, indices, batch, stage_metrics=False, refine=None):
    """This rank's share of the pairs through the device pipeline, `batch` pairs per chunk -> f32[k,4,4] (device), in the order of
    `indices`.  stage_metrics: also the per-stage metric rows against the data set's ground truth -> (poses, counts int32[k,7] on
    the device); the poses are the same.  refine: register_chunks' -> (..., refined dict) with the unrefined results unchanged."""
    idx = list(indices)
    return register_chunks(pipe, [idx[lo:lo + batch] for lo in range(0, len(idx), batch)],
                           lambda ch: items_batched(dataset, ch, pipe.device),
                           (lambda ch: [dataset.meta(i, pipe.device)['relt_pose'] for i in ch]) if stage_metrics else None, refine)


# ---------------------------------------------------------------------------------------------------- scoring
def dgr_summary(stats, recall_key='recall'):
    """stats [n,3]: evaluate.dgr_success rows (success, rte, rre) -> dict(pairs, <recall_key>, te, re); te / re are means over the
    successful pairs, NaN when there is none (test.py:278-284)."""
    st = np.array(stats, np.float64).reshape(-1, 3)
    good = st[:, 0] == 1
    return {'pairs': int(st.shape[0]), recall_key: float(good.mean()) if st.size else 0.0,
            'te': float(st[good, 1].mean()) if good.any() else float('nan'),
            're': float(st[good, 2].mean()) if good.any() else float('nan')}


def stage_report(scene_of, counts, P, fmr_ratio=0.05):
    """evaluate.stage_summary of all pairs and per scene (scene_of: one scene name per row of counts, data-set order)
    -> dict(overall figures..., per_scene={scene: figures})"""
    counts = np.asarray(counts).reshape(-1, 7)
    scene_of = np.asarray(list(scene_of), dtype=object)
    out = evaluate.stage_summary(counts, P, fmr_ratio)
    out['per_scene'] = {s: evaluate.stage_summary(counts[scene_of == s], P, fmr_ratio) for s in dict.fromkeys(scene_of.tolist())}
    return out


# ---------------------------------------------------------------------------------------------------- command line and main()
def add_common_args(ap, driver_name, batch_default, log_root_default, preset_note=''):
    """the options every driver takes; a driver adds its own and then calls parse_with_preset"""
    from .config import DRIVER_PRESETS
    ap.add_argument('--root', required=True)
    ap.add_argument('--preset', default=DRIVER_PRESETS[driver_name][0],
                    help='constants and weights (buffer_amd/config.py): ' + ', '.join(DRIVER_PRESETS[driver_name]) + preset_note)
    ap.add_argument('--batch', type=int, default=batch_default)
    ap.add_argument('--limits', default=None, help='frozen neighbourhood limits "a,b,c" (default: calibrate like dataloader.py:18-51)')
    ap.add_argument('--stage-metrics', action='store_true',
                    help='also compute the per-stage ground-truth metrics (repeatability, inlier ratio, FMR, consensus precision): '
                         'summary key "stage", per-pair rows in <log-root>/stage_metrics.json')
    ap.add_argument('--log-root', default=None, help=f'where the logs and stage_metrics.json go (default: {log_root_default})')
    ap.add_argument('--by-overlap', action='store_true',
                    help='also compute every pair\'s overlap under the ground truth (buffer_amd/pairs.py) and report pair count, DGR recall '
                         'and, with --stage-metrics, the stage figures per overlap band: summary key "by_overlap"')


def add_refine_args(ap):
    """--refine and its two settings: the dense refinement stage, the same on every driver (parse_with_preset adds them)"""
    from .ops import ICP_METHODS
    ap.add_argument('--refine', default=None, choices=sorted(ICP_METHODS) + ['voxelized'],
                    help='also refine every returned pose by dense ICP on the first-level clouds (BufferPipeline.refine_batch): summary '
                         'key "refined" = the figures of the refined poses + mean fitness / inlier_rmse / iterations; every other key '
                         'stays that of the unrefined poses.  voxelized: voxelized Generalized ICP on one voxel map of the targets '
                         '(the learned path only; "refined" also carries voxel and neighbors, its inlier_rmse is the distance to voxel means)')
    ap.add_argument('--refine-dist', type=float, default=None, help='correspondence distance of --refine (default: the preset\'s dist_th)')
    ap.add_argument('--refine-iters', type=int, default=30, help='most ICP iterations of --refine')
    ap.add_argument('--refine-voxel', type=float, default=None,
                    help='--refine voxelized: the voxel edge (default: twice the correspondence distance)')
    ap.add_argument('--refine-neighbors', type=int, default=7, choices=(1, 7, 27),
                    help='--refine voxelized: voxels met by a source point (the voxel it falls into, + its 6 face neighbours, or all 27)')
    ap.add_argument('--refine-normals', default='knn', choices=('knn', 'hybrid'),
                    help='the normals of --refine on the learned path.  knn: the 30 nearest neighbours (default).  hybrid: the 30 nearest '
                         'inside --refine-normal-radius, one launch without a retry loop (preprocess.estimate_normals_radius); '
                         'the summary carries "refine_normals", and "refined" its "refine_normal_radius"')
    ap.add_argument('--refine-normal-radius', type=float, default=None, metavar='R',
                    help='--refine-normals hybrid: the radius (default: twice the correspondence distance)')


def add_descriptor_args(ap):
    """--descriptor: the learned path or the classical baseline, the same on every driver (parse_with_preset adds it)"""
    ap.add_argument('--descriptor', default='buffer', choices=('buffer', 'fpfh'),
                    help='buffer: the learned path (default).  fpfh: the classical baseline on the same pairs, thresholds and logs -- FPFH on '
                         'the second-level clouds, mutual matches, RANSAC (buffer_amd/fpfh.py); no calibration, no --stage-metrics; the '
                         'summary carries "descriptor"')
    ap.add_argument('--estimator', default='ransac', choices=('ransac', 'fgr', 'sc2', 'clique'),
                    help='the pose estimator of --descriptor fpfh.  ransac: seeded 3-point hypotheses (default).  fgr: Fast Global Registration '
                         'on the same matches, one batched call per chunk (buffer_amd/fgr.py).  sc2: SC2-PCR, the deterministic second-order '
                         'spatial-compatibility consensus, one batched call per chunk (buffer_amd/sc2.py).  clique: greedy maximum clique of the '
                         'compatibility graph + truncated least squares, one batched call per chunk (buffer_amd/clique.py), also reporting '
                         '"certified_pairs" = the pairs whose clique reaches the k-core bound; the summary carries "estimator"')
    ap.add_argument('--keypoints', default='all', choices=('all', 'iss'),
                    help='the points --descriptor fpfh matches.  all: every point of the second-level clouds (default).  iss: their ISS '
                         'keypoints (buffer_amd/keypoints.py: salient radius 6 voxels, non-max radius 4 voxels); the summary carries '
                         '"keypoints" = the detector, the two radii and the mean keypoints per cloud')
    ap.add_argument('--match-ratio', type=float, default=None, metavar='R',
                    help="--descriptor fpfh: Lowe's ratio test on top of the mutual filter, 0 < R < 1 -- a match stays only if its nearest "
                         'descriptor distance is at most R times the second nearest (ops.feature_match; default: no ratio test); the '
                         'summary carries "match_ratio"')
    ap.add_argument('--fpfh-normals', default='given', choices=('given', 'hybrid'),
                    help='--descriptor fpfh: the normals under FPFH and its --refine.  given: the data set\'s (default).  hybrid: recomputed '
                         'from the 30 nearest points inside 2 voxels, oriented to the origin '
                         '(preprocess.estimate_normals_radius); the summary carries "fpfh_normals"')


def add_denoise_args(ap):
    """--denoise and its settings: outlier removal on the first-level clouds, the same on every driver (parse_with_preset adds them)"""
    ap.add_argument('--denoise', default=None, choices=('statistical', 'radius'),
                    help='remove outliers from every first-level cloud before the second voxel level (preprocess.prepare_fragments, '
                         'denoise=).  statistical: open3d remove_statistical_outlier, a point stays iff the mean distance to its '
                         '--denoise-neighbors nearest points is below the cloud\'s mean + --denoise-std-ratio standard deviations.  radius: '
                         'remove_radius_outlier, a point stays iff more than --denoise-neighbors points lie inside --denoise-radius; the '
                         'summary carries "denoise" = the method, its parameters and the mean removed fraction')
    ap.add_argument('--denoise-neighbors', type=int, default=None, metavar='N',
                    help='--denoise statistical: the neighbours of the mean distance, 1..64 (default 20); radius: the count to exceed (default 16)')
    ap.add_argument('--denoise-std-ratio', type=float, default=None, metavar='S', help='--denoise statistical: the ratio, > 0 (default 2.0)')
    ap.add_argument('--denoise-radius', type=float, default=None, metavar='R', help='--denoise radius: the ball radius, finite and > 0 (required)')


def denoise_option(a):
    """the parsed --denoise options -> prepare_fragments' `denoise` dict, None without --denoise"""
    if getattr(a, 'denoise', None) is None:
        return None
    if a.denoise == 'statistical':
        return dict(method='statistical', nb_neighbors=20 if a.denoise_neighbors is None else a.denoise_neighbors,
                    std_ratio=2.0 if a.denoise_std_ratio is None else a.denoise_std_ratio)
    return dict(method='radius', nb_points=16 if a.denoise_neighbors is None else a.denoise_neighbors, radius=a.denoise_radius)


def parse_with_preset(ap, argv, driver_name):
    """-> (args, Config of --preset); a preset of another data set is an argument error"""
    from .config import preset
    add_refine_args(ap)
    add_descriptor_args(ap)
    add_denoise_args(ap)
    a = ap.parse_args(argv)
    if a.denoise is None:
        for name in ('neighbors', 'std_ratio', 'radius'):
            if getattr(a, 'denoise_' + name) is not None:
                ap.error(f'--denoise-{name.replace("_", "-")} {getattr(a, "denoise_" + name)} is a setting of --denoise: it needs --denoise')
    if a.denoise == 'statistical' and a.denoise_radius is not None:
        ap.error(f'--denoise-radius {a.denoise_radius} is the ball of --denoise radius')
    if a.denoise == 'radius' and a.denoise_std_ratio is not None:
        ap.error(f'--denoise-std-ratio {a.denoise_std_ratio} is the ratio of --denoise statistical')
    if a.denoise == 'radius' and a.denoise_radius is None:
        ap.error('--denoise radius needs --denoise-radius')
    if a.denoise_radius is not None and not (0.0 < a.denoise_radius < float('inf')):
        ap.error(f'--denoise-radius {a.denoise_radius}: must be finite and > 0')
    if a.denoise_std_ratio is not None and not (0.0 < a.denoise_std_ratio < float('inf')):
        ap.error(f'--denoise-std-ratio {a.denoise_std_ratio}: must be finite and > 0')
    if a.denoise == 'statistical' and a.denoise_neighbors is not None and not (1 <= a.denoise_neighbors <= 64):
        ap.error(f'--denoise-neighbors {a.denoise_neighbors}: must be in 1..64 with --denoise statistical')
    if a.denoise == 'radius' and a.denoise_neighbors is not None and a.denoise_neighbors < 0:
        ap.error(f'--denoise-neighbors {a.denoise_neighbors}: must be >= 0')
    if a.descriptor == 'fpfh' and a.stage_metrics:
        ap.error('--stage-metrics measures the stages of the learned path: not available with --descriptor fpfh')
    if a.estimator != 'ransac' and a.descriptor != 'fpfh':
        ap.error(f'--estimator {a.estimator} chooses the estimator of the classical baseline: it needs --descriptor fpfh')
    if a.keypoints != 'all' and a.descriptor != 'fpfh':
        ap.error(f'--keypoints {a.keypoints} chooses the detector of the classical baseline: it needs --descriptor fpfh')
    if a.match_ratio is not None and a.descriptor != 'fpfh':
        ap.error(f'--match-ratio {a.match_ratio} thins the matches of the classical baseline: it needs --descriptor fpfh')
    if a.match_ratio is not None and not (0.0 < a.match_ratio < 1.0):
        ap.error(f'--match-ratio {a.match_ratio}: must be in (0, 1)')
    if a.fpfh_normals != 'given' and a.descriptor != 'fpfh':
        ap.error(f'--fpfh-normals {a.fpfh_normals} chooses the normals of the classical baseline: it needs --descriptor fpfh')
    if a.refine_normals != 'knn' and (not a.refine or a.descriptor == 'fpfh'):
        ap.error(f'--refine-normals {a.refine_normals} chooses the normals of --refine on the learned path: it needs --refine, and with '
                 '--descriptor fpfh the normals are those of --fpfh-normals')
    if a.refine_normal_radius is not None and a.refine_normals != 'hybrid':
        ap.error(f'--refine-normal-radius {a.refine_normal_radius} is the radius of --refine-normals hybrid')
    if a.refine_normal_radius is not None and not (0.0 < a.refine_normal_radius < float('inf')):
        ap.error(f'--refine-normal-radius {a.refine_normal_radius}: must be finite and > 0')
    if a.refine == 'voxelized' and a.descriptor == 'fpfh':
        ap.error('--refine voxelized refines the learned path: not available with --descriptor fpfh')
    if a.refine_voxel is not None and not (0.0 < a.refine_voxel < float('inf')):
        ap.error(f'--refine-voxel {a.refine_voxel}: must be finite and > 0')
    try:
        return a, preset(a.preset, driver_name)
    except ValueError as e:
        ap.error(str(e))


def init():
    """a driver's first GPU-touching call, before its data set is built -> (rank, world, device, collective device)"""
    from . import dist as bdist
    return bdist.init(int(os.environ.get('LOCAL_RANK', 0)))


def run(a, cfg, ds, ranks, *, summarize, dgr_thresholds, labels, log_root, calibrate_pairs, scene_of=None):
    """The body of a driver's main() once its data set exists: neighbourhood limits (--limits, or calibrated on the first
    `calibrate_pairs` pairs by rank 0 and broadcast), this rank's shard through register_pairs, gather, and on rank 0 the report:
    summarize(poses) -> the driver's own figures, the common ones, --by-overlap under the driver's (rte, rre) thresholds and
    --stage-metrics (per scene with scene_of = one scene name per pair; stage_metrics.json under log_root, pair ids = labels).
    --descriptor fpfh: fpfh.FpfhRegistration stands in for BufferPipeline (nothing to calibrate; the line carries "descriptor" and
    "estimator", --estimator choosing its RANSAC, its Fast Global Registration, its SC2-PCR or its max-clique + TLS estimator, which adds
    "certified_pairs"; --keypoints iss makes it match ISS keypoints instead of every point and adds "keypoints"; --match-ratio R
    adds Lowe's ratio test to its matching and "match_ratio"; --fpfh-normals hybrid recomputes its normals and adds "fpfh_normals").
    --refine: the refined poses travel in a second gather_poses and are summarized under "refined"; everything else reads the
    unrefined poses.  --refine-normals hybrid adds "refine_normals" (and "refined" its "refine_normal_radius").
    ranks: init()'s result.  Prints one JSON line and returns the poses f32[n,4,4] (numpy) on rank 0."""
    from . import dist as bdist
    from .pipeline import BufferPipeline
    rank, world, dev, cdev = ranks
    denoise = denoise_option(a)
    if denoise is not None:                                  # read by pack_pair / pack_pairs, which log the removed fractions
        ds.denoise, ds.denoise_log = denoise, []
    fpfh = getattr(a, 'descriptor', 'buffer') == 'fpfh'
    if fpfh:
        from .fpfh import FpfhRegistration
        iss = getattr(a, 'keypoints', 'all') == 'iss'
        pipe = FpfhRegistration(cfg, dev, estimator=getattr(a, 'estimator', 'ransac'),     # no neighbourhood limits: nothing to calibrate
                                keypoints='iss' if iss else None, match_ratio=getattr(a, 'match_ratio', None),
                                normals=getattr(a, 'fpfh_normals', 'given'))
    else:
        pipe = BufferPipeline(cfg, dev)
    if a.limits and not fpfh:
        pipe.limits = [int(x) for x in a.limits.split(',')]
    elif not fpfh:
        if rank == 0:                                        # dataloader.py:18-51 on the first pairs
            host = []
            for i in range(min(len(ds), calibrate_pairs)):
                s = ds.item(i, dev)
                host.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in s.items()})
            pipe.calibrate(host)
        pipe.limits = bdist.broadcast_limits(pipe.limits if rank == 0 else [0, 0, 0], device=cdev)
    ids = bdist.shard_indices(len(ds), rank, world)
    if denoise is not None:
        ds.denoise_log.clear()                               # (the calibration pairs come again below)
    t0 = time.perf_counter()
    refine = None
    if getattr(a, 'refine', None):
        refine = dict(method=a.refine, max_dist=cfg.dist_th if a.refine_dist is None else a.refine_dist, max_iteration=a.refine_iters)
        if a.refine == 'voxelized':
            rv = getattr(a, 'refine_voxel', None)
            refine.update(voxel=2.0 * refine['max_dist'] if rv is None else rv, neighbors=getattr(a, 'refine_neighbors', 7))
        if getattr(a, 'refine_normals', 'knn') != 'knn':
            rn = getattr(a, 'refine_normal_radius', None)
            refine.update(normals=a.refine_normals, normal_radius=2.0 * refine['max_dist'] if rn is None else rn)
    res = register_pairs(pipe, ds, ids, a.batch, stage_metrics=a.stage_metrics, refine=refine)
    refined = None
    if refine is not None:
        res, refined = (res[:-1] if a.stage_metrics else res[0]), res[-1]
    poses = bdist.gather_poses(ids, res[0] if a.stage_metrics else res, len(ds), device=cdev)
    if refined is not None:
        refined = bdist.gather_poses(ids, refined['poses'], len(ds), device=cdev, extra=torch.stack(
            [refined['fitness'].float(), refined['inlier_rmse'].float(), refined['iterations'].float()], 1))
    counts = bdist.gather_counts(ids, res[1].to(cdev), len(ds), device=cdev).cpu().numpy() if a.stage_metrics else None
    certified = None
    if fpfh and pipe.estimator == 'clique':                  # one flag per pair, in the order of ids (the chunks' order)
        flags = torch.cat(pipe.certified_log or [torch.zeros(0, dtype=torch.bool, device=dev)]).to(torch.int32).reshape(-1, 1)
        certified = bdist.gather_counts(ids, flags.to(cdev), len(ds), device=cdev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    poses = poses.cpu().numpy()
    if rank == 0:
        ref_out = None
        if refined is not None:                              # first: a summarize() that writes logs leaves those of the unrefined poses
            stats = refined[1].cpu().numpy().astype(np.float64)
            ref_out = dict(summarize(refined[0].cpu().numpy()), method=a.refine, max_dist=refine['max_dist'],
                           max_iteration=a.refine_iters, fitness=float(stats[:, 0].mean()) if len(stats) else 0.0,
                           inlier_rmse=float(stats[:, 1].mean()) if len(stats) else 0.0,
                           iterations=float(stats[:, 2].mean()) if len(stats) else 0.0)
            if a.refine == 'voxelized':
                ref_out.update(voxel=refine['voxel'], neighbors=refine['neighbors'])
            if 'normals' in refine:
                ref_out.update(refine_normal_radius=refine['normal_radius'])
        out = summarize(poses)
        out.update(pairs_per_sec=len(ds) / dt, n_gpus=world, limits=pipe.limits, preset=a.preset)
        if fpfh:
            out['descriptor'] = 'fpfh'
            out['estimator'] = getattr(a, 'estimator', 'ransac')
            if certified is not None:
                out['certified_pairs'] = int((certified == 1).sum())
            if pipe.match_ratio is not None:
                out['match_ratio'] = pipe.match_ratio
            if pipe.normals != 'given':
                out['fpfh_normals'] = pipe.normals
            if pipe.keypoints == 'iss':                      # (the mean is this rank's: the counts stay on the rank that found them)
                kc = np.concatenate(pipe.keypoint_counts_log or [np.zeros(0, np.int64)])
                out['keypoints'] = dict(detector='iss', salient_radius=pipe.iss_salient_radius, non_max_radius=pipe.iss_non_max_radius,
                                        mean_per_cloud=float(kc.mean()) if len(kc) else 0.0)
        if denoise is not None:                              # (the mean is this rank's: the fractions stay on the rank that found them)
            out['denoise'] = dict(denoise, removed=float(np.mean(ds.denoise_log)) if ds.denoise_log else 0.0)
        if ref_out is not None:
            out['refined'] = ref_out
            if 'normals' in refine:
                out['refine_normals'] = refine['normals']
        overlaps = None
        if a.by_overlap:
            from . import pairs
            out['by_overlap'], overlaps = pairs.overlap_report(ds, poses, dev, *dgr_thresholds, counts, cfg.num_keypts)
        if a.stage_metrics:
            out['stage'] = (evaluate.stage_summary(counts, cfg.num_keypts) if scene_of is None
                            else stage_report(scene_of, counts, cfg.num_keypts))
            evaluate.write_stage_metrics(os.path.join(log_root, 'stage_metrics.json'), labels, counts, cfg.num_keypts, out['stage'],
                                         overlaps)
        print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()
    return poses if rank == 0 else None
