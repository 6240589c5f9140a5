"""The classical baseline beside the learned path: FPFH descriptors (csrc/fpfh.hip, buf_fpfh), mutual nearest-neighbour matching
in descriptor space, 3-point correspondence RANSAC (buf_ransac_kabsch) and an optional ICP step -- in open3d terms
compute_fpfh_feature followed by registration_ransac_based_on_feature_matching.  open3d is absent here: the descriptor is restated
from its published form (include/buffer_hip.h, N6; parity unpinned).

    compute_fpfh        descriptors of one or several stacked clouds: one cell grid, one radius query, one launch pair
    match               (mutual) 1-NN matches of two descriptor sets through ops.knn (d = 33: the exact fp32 scan)
    match_batch         the same matches for all pairs of a batch in ONE ops.feature_match call (csrc/match.hip), optionally thinned
                        by Lowe's ratio test
    FpfhRegistration    estimator='ransac' (default), 'fgr' (buffer_amd/fgr.py: one batched Fast Global Registration call per
                        batch on the concatenated match lists), 'sc2' (buffer_amd/sc2.py: one batched SC2-PCR call per batch on the
                        same lists) or 'clique' (buffer_amd/clique.py: one batched max-clique + TLS call per batch on the same
                        lists); keypoints='iss': matching and the estimator on ISS keypoints (buffer_amd/keypoints.py) instead of every
                        point; register_batch / register_batches with the return shapes of pipeline.BufferPipeline, on the second-level
                        clouds and normals of driver.upload's dicts
"""
import numpy as np
import torch

from . import ops

ESTIMATORS = ('ransac', 'fgr')
ALL_ESTIMATORS = ESTIMATORS + ('sc2',)
KNOWN_ESTIMATORS = ALL_ESTIMATORS + ('clique',)
KEYPOINTS = (None, 'iss')
NORMALS = ('given', 'hybrid')


def compute_fpfh(points, normals, radius, max_nn=100, lengths=None, grid=None):
    """points, normals f32[n,3] (device; several clouds stacked when `lengths` int[nc] is given) -> FPFH f64[n,33]: the neighbours
    of a point are the max_nn nearest inside `radius` within its own cloud, itself included (open3d's KDTreeSearchParamHybrid).
    One CellGrid over the stacked clouds, one query with k = max_nn, one buf_fpfh call for all clouds.  grid: a CellGrid over the same
    points and lengths with a radius no smaller (shared with keypoints.iss_keypoints); the rows, and so the result, are the same."""
    points = ops._dev(points, torch.float32, "compute_fpfh.points")
    n = int(points.shape[0])
    lens = np.array([n], np.int32) if lengths is None else np.asarray(lengths, np.int32).reshape(-1)
    if int(lens.sum()) != n:
        raise ValueError(f"compute_fpfh: lengths sum to {int(lens.sum())}, points holds {n} rows")
    if not (2 <= int(max_nn) <= 128):
        raise ValueError(f"compute_fpfh: max_nn={max_nn} (2..128)")
    if n == 0:
        return torch.zeros((0, 33), dtype=torch.float64, device=points.device)
    if grid is None:
        grid = ops.CellGrid(points, lens, float(radius))
    elif grid.radius < float(radius) or grid.ns != n or not np.array_equal(grid.s_lengths, lens):
        raise ValueError("compute_fpfh: the given grid does not cover these clouds at this radius")
    nbr = grid.query(points, lens, int(max_nn), radius=float(radius), q_order=grid.order)
    return ops.fpfh(points, normals, nbr, int(max_nn))


def match(fa, fb, mutual=True):
    """fa f64|f32[na,d], fb [nb,d] (device) -> int32[m,2] rows (i, j): j = the nearest row of fb to fa[i] (ops.knn on the fp32
    casts, Euclidean, ties to the lowest row), ascending i.  mutual: only the rows whose i is also the nearest row of fa to fb[j]."""
    a, b = fa.float().contiguous(), fb.float().contiguous()
    if a.shape[0] == 0 or b.shape[0] == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=a.device)
    ab = ops.knn(b[None], a[None], 1)[1].reshape(-1)
    i = torch.arange(a.shape[0], device=a.device)
    if mutual:
        ba = ops.knn(a[None], b[None], 1)[1].reshape(-1)
        i = i[ba[ab] == i]
    return torch.stack([i, ab[i]], 1).to(torch.int32).contiguous()


def match_batch(F, lens, mutual=True, ratio=None):
    """F f64|f32[sum lens,d] (device): the descriptors of the clouds src, tgt, src, tgt, ... stacked as register_batch stacks them,
    lens int[2B] -> (corr int32[m,2] (device), corr_lengths int32[B] (host)): per pair the rows of match(F_src, F_tgt, mutual), the
    pairs concatenated -- one ops.feature_match call, one read-back (the counts).  ratio (None or in (0, 1)): Lowe's ratio test on the
    forward matches as well (nearest squared distance <= ratio^2 x the second nearest)."""
    lens = np.asarray(lens, np.int32).reshape(-1)
    if lens.shape[0] % 2:
        raise ValueError(f'match_batch: {lens.shape[0]} clouds do not pair up')
    F = F.float()
    if int(lens.sum()) != int(F.shape[0]):
        raise ValueError(f'match_batch: lengths sum to {int(lens.sum())}, F holds {int(F.shape[0])} rows')
    parts = torch.split(F, [int(n) for n in lens]) if len(lens) else ()
    empty = F[:0]
    fa, fb = torch.cat(parts[0::2] or (empty,)), torch.cat(parts[1::2] or (empty,))
    corr, cl, _, _ = ops.feature_match(fa, lens[0::2], fb, lens[1::2], mutual=mutual, ratio=ratio)
    return corr, cl


def ransac_on_matches(src, tgt, corr, nhyp, seed, max_dist, edge_similarity):
    """src f32[ns,3], tgt f32[nt,3], corr int32[m,2] (device) -> pose f32[4,4] src -> tgt: ops.ransac_kabsch over the matched rows
    (the kernel indexes both clouds with one list, so the rows are gathered first); fewer than 3 matches give the identity."""
    if corr.shape[0] < 3:
        return torch.eye(4, dtype=torch.float32, device=src.device)
    c = corr.long()
    idx = torch.arange(corr.shape[0], dtype=torch.int32, device=src.device)
    return ops.ransac_kabsch(src[c[:, 0]].contiguous(), tgt[c[:, 1]].contiguous(), idx, nhyp=int(nhyp), seed=int(seed) & ops._MASK64,
                             max_dist=float(max_dist), edge_similarity=float(edge_similarity))[0]


class FpfhRegistration:
    """FPFH + mutual matching + RANSAC (+ ICP) with BufferPipeline's calling convention.  radius = radius_factor * cfg.voxel_size_0
    (the usual 5 voxels), RANSAC inlier distance = dist_factor * cfg.voxel_size_0, cfg.ransac_hypotheses hypotheses.
    estimator='fgr': Fast Global Registration instead of the RANSAC, on the same matches and seeds, with the paper's delta = the same
    dist_factor * cfg.voxel_size_0 in the clouds' units and open3d's defaults otherwise.
    estimator='sc2': SC2-PCR on the same matches (no seeds: it is deterministic), with d_thr = inlier_thr = the same
    dist_factor * cfg.voxel_size_0, no non-maximum suppression and Sc2Options' defaults otherwise; a pair with more than
    ops.SC2_MAX_ROWS (16 384) matches is an error, not a truncation.
    estimator='clique': the max-clique + TLS estimator on the same matches (deterministic as well), with d_thr = tim_thr = inlier_thr =
    the same dist_factor * cfg.voxel_size_0, t_thr = half of it and CliqueOptions' defaults otherwise, under the same row limit; the
    last call's `certified` (bool[B]: the clique reaches the k-core bound) and `bound` (int32[B]) stay on the object, on the device.
    keypoints=None (default): every point is described and matched.  keypoints='iss': ISS keypoints (buffer_amd/keypoints.py) with the
    salient / non-max radii iss_salient_factor / iss_non_max_factor * cfg.voxel_size_0 (open3d's 6 x / 4 x resolution heuristic, the
    voxel size standing in for the resolution), iss_gamma = (gamma_21, gamma_32) and iss_min_neighbors; FPFH is still computed for
    every point, matching and the estimator then run on the keypoints' rows alone (fewer than 3 matches: the identity, as ever).
    iss_resolution='voxel' (default): those radii.  iss_resolution='estimate': the two factors times open3d's own resolution, the mean
    nearest-neighbour distance (preprocess.cloud_resolution) averaged over the clouds of the call: one more k = 2 search and one host
    wait per call; `iss_radii` keeps the last call's two radii.
    `keypoint_counts` keeps the last call's keypoints per cloud (int64[2B], host); refine_batch goes on refining on the dense clouds.
    match_ratio=None (default): the mutual matches as they are.  match_ratio=R in (0, 1): Lowe's ratio test on top (match_batch).  Either
    way all pairs of a batch are matched in one match_batch call, with the rows match() gives pair by pair.
    normals='given' (default): the normals that arrive with the second-level clouds (the data set's 30-NN ones).  normals='hybrid': they
    are recomputed from the normal_max_nn (30) nearest points inside normal_radius_factor (2) * cfg.voxel_size_0, oriented to the
    origin (preprocess.estimate_normals_radius: one grid of its own at that radius, one query, one launch -- FPFH's grid at 5 voxels
    would serve, but a query at 2 voxels on it measured 4.8 x the whole call on a grid of its own); refine_batch then refines
    with normals estimated in the same way."""

    def __init__(self, cfg, device='cuda:0', radius_factor=5.0, max_nn=100, dist_factor=1.5, edge_similarity=0.9, estimator='ransac',
                 keypoints=None, iss_salient_factor=6.0, iss_non_max_factor=4.0, iss_gamma=(0.975, 0.975), iss_min_neighbors=5,
                 match_ratio=None, normals='given', normal_radius_factor=2.0, normal_max_nn=30, iss_resolution='voxel'):
        self.cfg, self.device = cfg, torch.device(device)
        if iss_resolution not in ('voxel', 'estimate'):
            raise ValueError(f"FpfhRegistration: unknown iss_resolution {iss_resolution!r} (one of ('voxel', 'estimate'))")
        self.iss_resolution, self.iss_factors = iss_resolution, (float(iss_salient_factor), float(iss_non_max_factor))
        if normals not in NORMALS:
            raise ValueError(f'FpfhRegistration: unknown normals {normals!r} (one of {NORMALS})')
        self.normals, self.normal_radius, self.normal_max_nn = normals, float(normal_radius_factor) * cfg.voxel_size_0, int(normal_max_nn)
        if match_ratio is not None and not (0.0 < float(match_ratio) < 1.0):
            raise ValueError(f'FpfhRegistration: match_ratio={match_ratio} (None, or in (0, 1))')
        self.match_ratio = None if match_ratio is None else float(match_ratio)
        if keypoints not in KEYPOINTS:
            raise ValueError(f'FpfhRegistration: unknown keypoints {keypoints!r} (one of {KEYPOINTS})')
        self.keypoints = keypoints
        self.iss_salient_radius = float(iss_salient_factor) * cfg.voxel_size_0
        self.iss_non_max_radius = float(iss_non_max_factor) * cfg.voxel_size_0
        self.iss_gamma, self.iss_min_neighbors = (float(iss_gamma[0]), float(iss_gamma[1])), int(iss_min_neighbors)
        self.keypoint_counts = None          # keypoints='iss': int64[2B] per-cloud keypoints of the last register_batch call (host)
        self.keypoint_counts_log = []        # and of every call so far, in call order (the drivers average it)
        if self.device.type != 'cuda':
            raise RuntimeError('FpfhRegistration runs on a HIP device only (no CPU path)')
        if estimator not in KNOWN_ESTIMATORS:
            raise ValueError(f'FpfhRegistration: unknown estimator {estimator!r} (one of {KNOWN_ESTIMATORS})')
        self.estimator = estimator
        self.certified = self.bound = None   # estimator='clique': of the last register_batch call
        self.certified_log = []              # and `certified` of every call so far, in call order (the drivers count it)
        self.radius = float(radius_factor) * cfg.voxel_size_0
        self.max_nn, self.max_dist, self.edge_similarity = int(max_nn), float(dist_factor) * cfg.voxel_size_0, float(edge_similarity)
        self.limits = None                   # the neighbourhood limits of the learned path: nothing to calibrate here

    def calibrate(self, samples):
        return self.limits

    @staticmethod
    def _clouds(inp):
        ns = int(inp['lengths'][0])
        return inp['points'][:ns], inp['points'][ns:], inp['features'][:ns, :3], inp['features'][ns:, :3]

    @torch.no_grad()
    def register_batch(self, inps, seeds=None, metrics_gt=None):
        """inps: list of driver.upload dicts -> list of pose f32[4,4] device tensors (src -> tgt), pair b seeded with seeds[b]."""
        if metrics_gt is not None:
            raise NotImplementedError('FpfhRegistration: the per-stage metrics belong to the learned path (keypoints, patches)')
        B = len(inps)
        if B == 0:
            return []
        seeds = list(range(B)) if seeds is None else list(seeds)
        pts = torch.cat([i['points'] for i in inps]).float().contiguous()
        nrm = torch.cat([i['features'][:, :3] for i in inps]).float().contiguous()
        lens = np.concatenate([np.asarray(i['lengths'], np.int32).reshape(2) for i in inps])
        if self.normals == 'hybrid':
            nrm = self._hybrid_normals(pts, lens)
        if self.keypoints == 'iss':
            pts, lens, F = self._iss_sets(pts, nrm, lens)
        else:
            F = compute_fpfh(pts, nrm, self.radius, self.max_nn, lens)
        off = np.concatenate([[0], np.cumsum(lens)])
        if self.estimator == 'fgr':
            return self._fgr_batch(pts, lens, off, F, seeds)
        if self.estimator == 'sc2':
            return self._sc2_batch(pts, lens, off, F)
        if self.estimator == 'clique':
            return self._clique_batch(pts, lens, off, F)
        corr, cl = match_batch(F, lens, True, self.match_ratio)
        co = np.concatenate([[0], np.cumsum(cl)])
        out = []
        for b in range(B):
            s0, t0, t1 = int(off[2 * b]), int(off[2 * b + 1]), int(off[2 * b + 2])
            out.append(ransac_on_matches(pts[s0:t0], pts[t0:t1], corr[int(co[b]):int(co[b + 1])], self.cfg.ransac_hypotheses, seeds[b],
                                         self.max_dist, self.edge_similarity))
        return out

    def _hybrid_normals(self, pts, lens):
        """normals='hybrid': the normals of the stacked clouds, oriented to the origin"""
        from . import preprocess
        return preprocess.estimate_normals_radius(pts, self.normal_radius, self.normal_max_nn, lengths=lens)

    def _iss_sets(self, pts, nrm, lens):
        """keypoints='iss': FPFH of EVERY point (a descriptor needs the SPFH of all its neighbours) and the ISS keypoints on one shared
        grid, then the keypoints' coordinates and descriptor rows -> (points f32[K,3], per-cloud keypoint counts int32[2B], F f64[K,33]):
        what matching and the estimators then see in place of the dense clouds"""
        from . import keypoints
        r_sal, r_nms = self.iss_salient_radius, self.iss_non_max_radius
        if self.iss_resolution == 'estimate':
            from . import preprocess
            res = preprocess.cloud_resolution(pts, lens)
            res = float(res[torch.isfinite(res)].mean().item()) if bool(torch.isfinite(res).any()) else self.cfg.voxel_size_0
            r_sal, r_nms = self.iss_factors[0] * res, self.iss_factors[1] * res
        self.iss_radii = (r_sal, r_nms)
        grid = ops.CellGrid(pts, lens, max(self.radius, r_sal, r_nms))
        F = compute_fpfh(pts, nrm, self.radius, self.max_nn, lens, grid=grid)
        idx, counts = keypoints.iss_keypoints(pts, r_sal, r_nms, self.iss_gamma[0], self.iss_gamma[1],
                                              self.iss_min_neighbors, lengths=lens, grid=grid)
        self.keypoint_counts = counts
        self.keypoint_counts_log.append(counts)
        return pts[idx].contiguous(), counts.astype(np.int32), F[idx].contiguous()

    def _batch_matches(self, pts, lens, off, F):
        """the matches of every pair (one match_batch call: the rows the RANSAC path gets) and the two sides stacked apart (the pairs'
        clouds alternate in pts: src, tgt, src, ...) -> (src, tgt, corr int32[m,2], corr_lengths int32[B] on the host)"""
        B = len(lens) // 2
        corr, cl = match_batch(F, lens, True, self.match_ratio)
        src = torch.cat([pts[int(off[2 * b]):int(off[2 * b + 1])] for b in range(B)])
        tgt = torch.cat([pts[int(off[2 * b + 1]):int(off[2 * b + 2])] for b in range(B)])
        return src, tgt, corr, cl

    def _sc2_batch(self, pts, lens, off, F):
        """the matches of every pair, then ONE sc2_batched call for the batch"""
        from . import sc2
        src, tgt, corr, cl = self._batch_matches(pts, lens, off, F)
        res = sc2.sc2_registration(src, lens[0::2], tgt, lens[1::2], corr, cl,
                                   d_thr=self.max_dist, inlier_thr=self.max_dist, nms_radius=0.0)
        return list(res['poses'].float().unbind(0))

    def _clique_batch(self, pts, lens, off, F):
        """the matches of every pair, then ONE clique_batched call for the batch; keeps its `certified` and `bound`"""
        from . import clique
        src, tgt, corr, cl = self._batch_matches(pts, lens, off, F)
        res = clique.clique_registration(src, lens[0::2], tgt, lens[1::2], corr, cl,
                                         d_thr=self.max_dist, tim_thr=self.max_dist, t_thr=self.max_dist / 2, inlier_thr=self.max_dist)
        self.certified, self.bound = res['certified'], res['bound']
        self.certified_log.append(self.certified)
        return list(res['poses'].float().unbind(0))

    def _fgr_batch(self, pts, lens, off, F, seeds):
        """the matches of every pair, then ONE fgr_batched call for the batch"""
        from . import fgr
        src, tgt, corr, cl = self._batch_matches(pts, lens, off, F)
        res = fgr.fast_global_registration(src, lens[0::2], tgt, lens[1::2], corr, cl,
                                           seeds=[int(s) & ops._MASK64 for s in seeds], maximum_correspondence_distance=self.max_dist,
                                           delta_absolute=True)
        return list(res['poses'].float().unbind(0))

    @torch.no_grad()
    def refine_batch(self, inps, poses, method='point_to_plane', max_dist=None, max_iteration=30, epsilon=1e-3):
        """One batched ICP call (ops.icp_batched, the device form BufferPipeline.refine_batch uses) on the same second-level clouds
        and their normals, started from `poses` -> BufferPipeline.refine_batch's dict."""
        if method not in ops.ICP_METHODS:
            raise ValueError(f'refine_batch: unknown method {method!r} (one of {sorted(ops.ICP_METHODS)})')
        dev, B = self.device, len(inps)
        if isinstance(poses, (list, tuple)):
            poses = torch.stack(list(poses)) if B else torch.zeros((0, 4, 4), device=dev)
        T0 = poses.to(dev, torch.float64).reshape(B, 4, 4).contiguous()
        if B == 0:
            return dict(poses=torch.zeros((0, 4, 4), dtype=torch.float32, device=dev), fitness=torch.zeros(0, dtype=torch.float64, device=dev),
                        inlier_rmse=torch.zeros(0, dtype=torch.float64, device=dev), iterations=torch.zeros(0, dtype=torch.int32, device=dev))
        cl = [self._clouds(i) for i in inps]
        sl, tl = np.array([c[0].shape[0] for c in cl], np.int32), np.array([c[1].shape[0] for c in cl], np.int32)
        src, tgt = torch.cat([c[0] for c in cl]).float().contiguous(), torch.cat([c[1] for c in cl]).float().contiguous()
        snrm = torch.cat([c[2] for c in cl]).float().contiguous() if method == 'generalized' else None
        tnrm = torch.cat([c[3] for c in cl]).float().contiguous() if method != 'point_to_point' else None
        if self.normals == 'hybrid' and method == 'generalized':
            nrm = self._hybrid_normals(torch.cat([src, tgt]), np.concatenate([sl, tl]))
            snrm, tnrm = nrm[:src.shape[0]].contiguous(), nrm[src.shape[0]:].contiguous()
        elif self.normals == 'hybrid' and method == 'point_to_plane':
            tnrm = self._hybrid_normals(tgt, tl)
        T, fit, rmse, iters, _ = ops.icp_batched(src, sl, tgt, tl, float(self.cfg.dist_th if max_dist is None else max_dist), T0, method,
                                                 tnrm, int(max_iteration), src_normals=snrm, epsilon=epsilon)
        return dict(poses=T.float(), fitness=fit, inlier_rmse=rmse, iterations=iters)

    @torch.no_grad()
    def register_batches(self, batches, seeds=None, metrics_gt=None, refine=None):
        """BufferPipeline.register_batches' shapes: batches = lists of upload dicts (or callables returning one) -> per batch the list
        of poses, or with refine=dict(method, max_dist, max_iteration) the tuple (poses, refine_batch's dict)."""
        if metrics_gt is not None:
            raise NotImplementedError('FpfhRegistration: the per-stage metrics belong to the learned path (keypoints, patches)')
        seeds = [None] * len(batches) if seeds is None else seeds
        out = []
        for b, s in zip(batches, seeds):
            inps = b() if callable(b) else b
            res = self.register_batch(inps, s)
            out.append(res if refine is None else (res, self.refine_batch(inps, res, **refine)))
        return out
