"""End-to-end registration of one fragment pair on one GPU (the inference branch of buffer.forward,
models/BUFFER.py:231-333, with the collate stage of ThreeDMatch/dataloader.py:115-245 moved on device)."""
import os
import time

import numpy as np
import torch

from . import ops, pyramid, registration
from .config import THREEDMATCH
from .patch_embedder import PatchEmbedder
from .point_learner import PointLearner, orient_axes
from .weights import load_weights

REFINE_NORMALS = ('knn', 'hybrid')       # refine_batch: how the dense clouds' normals are estimated


class BufferPipeline:
    def __init__(self, cfg=THREEDMATCH, device='cuda:0', weights=None, limits=None):
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('BufferPipeline runs on a HIP device only (no CPU path)')
        W = weights if weights is not None else load_weights(cfg.weights)
        self.W = W
        self.point = PointLearner(W, self.device, cfg.scale)
        self.desc = PatchEmbedder(W, self.device, cfg)
        self.inlier = registration.CostVolume(W, self.device, cfg.azi_n, getattr(cfg, 'cnn_arith', 'f32'))
        self.limits = None if limits is None else [int(x) for x in limits]
        self.host_wait_s = 0.0        # seconds the enqueueing thread spent blocked in the path's host round trips (diagnostics)

    def check_range(self):
        """cnn_arith='split': the kernels are safe by construction (csrc/split_safe.hip: every patch / match whose values leave the f16
        range is recomputed by the fp32 kernel in the same stream), so there is nothing to check and no synchronisation here.  Only a
        split network without an fp32 kernel for its widths (never the released ones) keeps the round-5 contract: FloatingPointError
        if its status word was set."""
        for m in (self.desc.fused, self.inlier.fused):
            if hasattr(m, 'check_range') and not getattr(m, 'safe', False):
                m.check_range()

    def range_fallbacks(self):
        """(patches, matches) of the LAST launches that left the f16 range and took the fp32 kernels (cnn_arith='split'; synchronises)"""
        return tuple(m.range_fallbacks() if hasattr(m, 'range_fallbacks') else 0 for m in (self.desc.fused, self.inlier.fused))

    def calibrate(self, samples):
        self.limits = [int(x) for x in pyramid.calibrate_limits(samples, self.cfg, self.device)]
        return self.limits

    def upload(self, sample):
        """host sample dict -> device-resident inputs (what the timed region of bench.py starts from)."""
        pts, lens, feats, src_raw, tgt_raw = pyramid.stack_sample(sample, self.device)
        return dict(points=pts, lengths=lens, features=feats, src_raw=src_raw, tgt_raw=tgt_raw)

    @torch.no_grad()
    def register(self, inp, seed=0, perms=None, detail=False, metrics_gt=None, tau_kp=None, tau_match=None, dist_th=None):
        """inp from upload() -> pose f32[4,4] (src -> tgt), device tensor: register_batch at one pair, the same launches.
        metrics_gt: the pair's ground-truth 4x4 (src -> tgt) -> (pose, counts int32[7] on the device), the pair's row of the
        per-stage metrics (register_batch).  The pose is the same.
        detail=True -> (pose, dict): what the stages held for this pair (_pair_detail), the metric row under 'stage_counts'.  A pair
        answered with the identity because a cloud has no keypoint leaves the dict empty otherwise; one with fewer than 3 mutual
        matches leaves it without the hypothesis keys."""
        met = None if metrics_gt is None else self._metric_args([metrics_gt], tau_kp, tau_match, dist_th)
        st, res = self._stages([inp], [seed], None if perms is None else [perms], met, detail)
        self.check_range()
        (pose,), counts = (res, None) if met is None else res
        if not detail:
            return pose if met is None else (pose, counts[0])
        out = self._pair_detail(st)
        if met is not None:
            out['stage_counts'] = counts[0]
        return pose, out

    @torch.no_grad()
    def register_batch(self, inps, seeds=None, perms=None, metrics_gt=None, tau_kp=None, tau_match=None, dist_th=None):
        """Several pairs through ONE set of launches per stage (the MI355X-native form: the pyramid, the VN
        blocks, FPS (one workgroup per cloud), patch selection, voxelisation, both CNNs and the 1-NN search all take the
        stacked batch; only the per-pair pose recovery loops).  inps: list of upload() dicts ->
        list of pose f32[4,4] device tensors.  A pair's result does not depend on what it is stacked with (register() is this
        path at one pair; tests/pair_chain.py is the independent pair-by-pair chain the tests hold both against).

        metrics_gt: the B ground-truth poses (src -> tgt, [B,4,4] or a list of 4x4; host or device) switches the per-stage
        metrics on -> (poses, counts), counts int32[B,7] ON THE DEVICE (columns ops.METRIC_COLUMNS: rep_src, rep_tgt, nn_inl,
        mutual, mutual_inl, cons, cons_true; evaluate.stage_summary turns host rows into ratios).  One more kernel
        (buf_match_metrics) is enqueued after pose recovery on the same stream, from the keypoints and 1-NN rows the batch already
        holds; nothing is read back here (.cpu() is the caller's) and the poses are bit-identical to a call without metrics_gt.
        A pair that never reaches matching -- a cloud with no point above keypts_th, or fewer than 3 mutual matches, i.e. the
        pairs answered with the identity -- gets -1 in every column ("not evaluated", as opposed to a count of zero).
        tau_kp (repeatability distance) and tau_match (match inlier distance) default to cfg.dist_th, the inlier distance of the
        configuration's data set; dist_th (consensus distance of the returned pose) is cfg.dist_th unless overridden."""
        met = None if metrics_gt is None else self._metric_args(metrics_gt, tau_kp, tau_match, dist_th, len(inps))
        _, res = self._stages(inps, seeds, perms, met)
        self.check_range()
        return res

    @torch.no_grad()
    def refine_batch(self, inps, poses, method='generalized', max_dist=None, max_iteration=30, epsilon=1e-3, voxel=None, neighbors=7,
                     normals='knn', normal_radius=None, normal_max_nn=30):
        """Dense refinement of a batch's poses: ONE batched ICP call (icp.py / csrc/icp.hip, all pairs in one set of launches) on the
        dense first-level clouds of inps (src_raw / tgt_raw), started from `poses` (B src -> tgt 4x4: what register_batch returned, a
        list or a [B,4,4] tensor), which are converted to f64 on the device -- no pose passes through the host.
        method: 'generalized' (plane-to-plane, epsilon = the covariance along a normal), 'point_to_plane' or 'point_to_point';
        max_dist: the correspondence distance, cfg.dist_th unless given.  Normals come from ONE stacked
        preprocess.estimate_normals(knn=30, orient=False, lengths=) call: of all 2B clouds (sources, then targets) for 'generalized', of
        the B targets for 'point_to_plane', none for 'point_to_point'.  normals='hybrid': the same clouds' normals from ONE
        preprocess.estimate_normals_radius call instead (the normal_max_nn nearest inside normal_radius, twice the correspondence
        distance unless given: one grid, one query, one launch, no retry and no host wait); the rest is unchanged.
        method 'voxelized' (icp.vgicp_batched, csrc/vgicp.hip): the normals of 'generalized', ONE voxel map of the B targets (voxel:
        its edge, twice the correspondence distance unless given; epsilon) and one batched call on it with `neighbors` (1, 7 or 27)
        voxels per source point; no nearest-neighbour search.  Its inlier_rmse is the distance to voxel means: of the order of the
        voxel size, not comparable with the other methods'.
        -> dict of device tensors: poses f32[B,4,4], fitness f64[B], inlier_rmse f64[B], iterations int32[B].
        Host waits: the normal estimation's own round trips and ICP's one int per 8 rounds ('voxelized': and the map's one record)."""
        from . import preprocess
        if method != 'voxelized' and method not in ops.ICP_METHODS:
            raise ValueError(f"refine_batch: unknown method {method!r} (one of {sorted(list(ops.ICP_METHODS) + ['voxelized'])})")
        if method == 'voxelized' and neighbors not in ops.VGICP_NEIGHBORS:
            raise ValueError(f'refine_batch: neighbors={neighbors} (one of {ops.VGICP_NEIGHBORS})')
        if normals not in REFINE_NORMALS:
            raise ValueError(f'refine_batch: unknown normals {normals!r} (one of {REFINE_NORMALS})')
        dev, B = self.device, len(inps)
        if isinstance(poses, (list, tuple)):
            poses = torch.stack(list(poses)) if B else torch.zeros((0, 4, 4), device=dev)
        T0 = poses.to(dev, torch.float64).reshape(B, 4, 4).contiguous()
        if B == 0:
            return dict(poses=torch.zeros((0, 4, 4), dtype=torch.float32, device=dev), fitness=torch.zeros(0, dtype=torch.float64, device=dev),
                        inlier_rmse=torch.zeros(0, dtype=torch.float64, device=dev), iterations=torch.zeros(0, dtype=torch.int32, device=dev))
        if normals == 'hybrid':
            nr = 2.0 * float(self.cfg.dist_th if max_dist is None else max_dist) if normal_radius is None else float(normal_radius)
            estimate = lambda pts, lengths: preprocess.estimate_normals_radius(pts, nr, int(normal_max_nn), orient=False, lengths=lengths)
        else:
            estimate = lambda pts, lengths: preprocess.estimate_normals(pts, knn=30, orient=False, lengths=lengths)
        srcs, tgts = [i['src_raw'][:, :3] for i in inps], [i['tgt_raw'][:, :3] for i in inps]
        sl, tl = np.array([s.shape[0] for s in srcs], np.int32), np.array([t.shape[0] for t in tgts], np.int32)
        src, tgt = torch.cat(srcs).float().contiguous(), torch.cat(tgts).float().contiguous()
        snrm = tnrm = None
        if method in ('generalized', 'voxelized'):
            nrm = estimate(torch.cat([src, tgt]), np.concatenate([sl, tl]))
            snrm, tnrm = nrm[:src.shape[0]].contiguous(), nrm[src.shape[0]:].contiguous()
        elif method == 'point_to_plane':
            tnrm = estimate(tgt, tl)
        if method == 'voxelized':
            edge = float(voxel) if voxel is not None else 2.0 * float(self.cfg.dist_th if max_dist is None else max_dist)
            vmap = ops.voxel_map_build(tgt, tl, edge, tnrm, epsilon)
            T, fit, rmse, iters, _ = ops.vgicp_batched(src, sl, vmap, T0, int(neighbors), snrm, None, int(max_iteration))
            return dict(poses=T.float(), fitness=fit, inlier_rmse=rmse, iterations=iters)
        T, fit, rmse, iters, _ = ops.icp_batched(src, sl, tgt, tl, float(self.cfg.dist_th if max_dist is None else max_dist), T0, method,
                                                 tnrm, int(max_iteration), src_normals=snrm, epsilon=epsilon)
        return dict(poses=T.float(), fitness=fit, inlier_rmse=rmse, iterations=iters)

    @torch.no_grad()
    def register_batches(self, batches, seeds=None, metrics_gt=None, tau_kp=None, tau_match=None, dist_th=None, refine=None):
        """A sequence of batches, software-pipelined over two HIP streams: the keypoint stage of batch i+1 (pyramid, point
        learner, FPS -- short kernels, FPS latency-bound on 2B of the 256 CUs) is enqueued on a high-priority side stream
        BEFORE the descriptor / matching stage of batch i goes onto the current stream, so it runs beside the chip-filling
        CNN kernels instead of in front of them.  Results are those of register_batch batch by batch.
        batches: list of lists of upload() dicts -- or of callables returning such a list, which are then evaluated on the side
        stream as part of the keypoint stage (device pre-processing of the next batch beside the CNN kernels of this one);
        seeds: list of lists -> list of lists of poses.
        metrics_gt: one entry per batch, each the batch's ground-truth poses as in register_batch (or a callable returning them,
        evaluated when the batch is) -> list of (poses, counts int32[B,7] on the device) per batch; the metric kernel of a batch
        follows its pose recovery on the current stream, so the two-stream overlap is as without it.
        refine: None, or the keyword arguments of refine_batch (method, max_dist, max_iteration, epsilon) -> every list entry becomes
        (the entry as without refine, refine_batch's dict for the batch): the refinement of batch i is enqueued on the current stream
        after its pose recovery (and metric kernel), from the poses that entry holds.  The unrefined poses and the metric rows keep
        their bits; ICP's readbacks block the enqueueing thread, so less of batch i+1 overlaps.  None: no launch, nothing allocated."""
        dev = self.device
        main = torch.cuda.current_stream(dev)
        if not hasattr(self, '_kp_stream'):
            self._kp_stream = torch.cuda.Stream(device=dev, priority=int(os.environ.get('BUF_KP_STREAM_PRIORITY', -1)))
        side = self._kp_stream
        seeds = [None] * len(batches) if seeds is None else seeds
        out = []

        def stage1(i):
            with torch.cuda.stream(side):
                inps = batches[i]() if callable(batches[i]) else batches[i]
                met = None
                if metrics_gt is not None:                 # (uploaded before the keypoint stage is queued: the copy waits for nothing)
                    gt = metrics_gt[i]() if callable(metrics_gt[i]) else metrics_gt[i]
                    met = self._metric_args(gt, tau_kp, tau_match, dist_th, len(inps))
                st = self._keypoints(inps, seeds[i], None)
                if met is not None:
                    st['metrics'] = met
                    st['cross'] = tuple(st.get('cross', ())) + (met['gt'],)
                if callable(batches[i]):                   # inputs made on the side stream are read on the current one too
                    st['cross'] = tuple(st.get('cross', ())) + tuple(v for x in inps for v in x.values() if isinstance(v, torch.Tensor))
                ev = torch.cuda.Event()
                ev.record(side)
            return st, ev

        side.wait_stream(main)
        nxt = stage1(0) if batches else None
        for i in range(len(batches)):
            st, ev = nxt
            main.wait_event(ev)
            for t in st.get('cross', ()):                  # produced on the side stream, consumed on the current one
                t.record_stream(main)
            st = self._describe(st)                        # ~300 ms of CNN work queued on the current stream, no host sync
            # the next batch's keypoint stage goes out NOW: its host round trip (per-cloud candidate counts) waits on the
            # side stream only, while the current stream is busy with the kernels queued above
            nxt = stage1(i + 1) if i + 1 < len(batches) else None
            res = self._match(st)
            if refine is not None:
                res = (res, self.refine_batch(st['inps'], res if metrics_gt is None else res[0], **refine))
            out.append(res)
        self.check_range()
        return out

    def _stages(self, inps, seeds, perms, met=None, detail=False):
        """the three stages of a stacked batch back to back -> (their state, what _match returns)"""
        st = self._keypoints(inps, seeds, perms, detail)
        if met is not None:
            st['metrics'] = met
        return st, self._match(self._describe(st))

    def _keypoints(self, inps, seeds, perms, detail=False):
        """pyramid -> point learner -> threshold -> FPS for a stacked batch -> state for _describe.
        detail: the stages also leave what register(detail=True) reports under st['detail'] (references only: no launch is added or
        moved)."""
        cfg, dev = self.cfg, self.device
        B = len(inps)
        if self.limits is None:
            raise RuntimeError('neighbourhood limits not calibrated: call calibrate() or pass limits=')
        seeds = list(range(B)) if seeds is None else list(seeds)
        lens = np.concatenate([np.asarray(i['lengths'], np.int32) for i in inps])            # [2B]
        pts = torch.cat([i['points'] for i in inps]) if B > 1 else inps[0]['points']
        feats = torch.cat([i['features'] for i in inps]) if B > 1 else inps[0]['features']
        w0 = ops.HOST_WAIT_S[0]
        pyr = pyramid.build_pyramid(pts, lens, self.limits, cfg)
        self.host_wait_s += ops.HOST_WAIT_S[0] - w0                                         # the two subsample row-count round trips
        pair_rows = lens.reshape(B, 2).sum(1)
        seg = pair_rows.astype(np.int32) if B > 1 else None      # InstanceNorm segments of the score heads: one per pair
        axis, eps, bottle, skips, _ = self.point.efcnn(pyr, feats, seg)
        score = self.point.detnet(pyr, bottle, skips, seg)
        pts0 = pyr['points'][0]
        cloud_len = torch.from_numpy(lens.astype(np.int64)).to(dev)
        cloud_id = torch.repeat_interleave(torch.arange(2 * B, device=dev), cloud_len)
        axis_o = orient_axes(axis, pts0)                                                    # BUFFER.py:244-249 (row-wise)
        t0 = time.perf_counter()                                                            # host round trip 1: the compaction sizes its
        keep = ops.compact_greater(score[:, 0], cfg.keypts_th).long()                        # output (:255-259, ascending), then the
        counts = torch.bincount(cloud_id[keep], minlength=2 * B).cpu().numpy()               # candidate counts per cloud for FPS
        self.host_wait_s += time.perf_counter() - t0
        st = dict(inps=inps, seeds=seeds, perms=perms, B=B)
        if (counts == 0).any():                             # rare: some cloud has no point above the threshold
            st['starved'] = set(int(c) // 2 for c in np.nonzero(counts == 0)[0])
            return st
        cand_p, cand_a = pts0[keep].contiguous(), axis_o[keep].contiguous()
        fps = ops.furthest_point_sample_ragged(cand_p, counts, cfg.num_keypts).long()       # one workgroup per cloud
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)).to(dev)
        gidx = (fps + off[:, None]).reshape(-1)
        st['kp'], st['ka'] = cand_p[gidx].contiguous(), cand_a[gidx].contiguous()           # [2B*P, 3]
        st['cross'] = (st['kp'], st['ka'])
        if detail:
            st['detail'] = dict(pyr=pyr, axis=axis, eps=eps, score=score)
        return st

    def _describe(self, st):
        """patch selection, voxelisation, descriptor CNN and the two 1-NN searches of a stacked batch: everything up to
        the first host round trip of the stage (the match count), enqueued without blocking."""
        cfg, dev = self.cfg, self.device
        inps, seeds, perms, B = st['inps'], st['seeds'], st['perms'], st['B']
        if 'starved' in st:                                 # the healthy pairs as a batch of their own, the identity for the others
            good = [b for b in range(B) if b not in st['starved']]
            met = st.get('metrics')
            poses = [torch.eye(4, device=dev) for _ in range(B)]       # ThreeDMatch/test.py:242-245: failed pair -> identity
            counts = None if met is None else torch.full((B, len(ops.METRIC_COLUMNS)), -1, dtype=torch.int32, device=dev)  # not evaluated
            if good:
                res = self._stages([inps[b] for b in good], [seeds[b] for b in good], None if perms is None else [perms[b] for b in good],
                                   None if met is None else dict(met, gt=met['gt'][good]))[1]
                sub, rows = (res, None) if met is None else res
                for b, p in zip(good, sub):
                    poses[b] = p
                if met is not None:
                    counts[good] = rows
            st['poses'] = poses if met is None else (poses, counts)
            return st
        kp, ka = st['kp'], st['ka']
        P = cfg.num_keypts
        raws = [r for i in inps for r in (i['src_raw'], i['tgt_raw'])]
        if perms is not None:
            sup = torch.cat([raws[2 * b + j][perms[b][j]] for b in range(B) for j in range(2)]).contiguous()
            sup_len = [r.shape[0] for r in raws]
        else:                                               # one launch shuffles every cloud of the step (keyed per pair seed)
            sup, sup_len = ops.permute_clouds(raws, [ops.perm_key(seeds[b], j) for b in range(B) for j in range(2)])
        patches = ops.select_patches_batched(sup, sup_len, kp, P, cfg.des_r, cfg.num_points_per_patch)   # one grid, one launch
        emb = self.desc.embed_patches(patches, ka, want_patches='detail' in st)
        desc = emb['desc'].view(B, 2, P, -1)
        _, s_idx = ops.knn(desc[:, 1].contiguous(), desc[:, 0].contiguous(), 1)            # BUFFER.py:347: ref = tgt
        _, t_idx = ops.knn(desc[:, 0].contiguous(), desc[:, 1].contiguous(), 1)
        s_nn, t_nn = s_idx[:, :, 0], t_idx[:, :, 0]
        st['mutual'] = t_nn.gather(1, s_nn) == torch.arange(P, device=dev)[None]
        st['s_nn'], st['t_nn'], st['emb'] = s_nn, t_nn, emb
        return st

    def _match(self, st):
        """mutual matches (first host round trip) -> cost volume -> pose recovery of all pairs in one set of launches
        (-> per-stage metric rows) -> list of B poses, or (poses, counts int32[B,7]) with metrics."""
        if 'poses' in st:
            return st['poses']
        cfg, dev = self.cfg, self.device
        seeds, B, kp, emb, s_nn, P = st['seeds'], st['B'], st['kp'], st['emb'], st['s_nn'], self.cfg.num_keypts
        poses = [None] * B
        t0 = time.perf_counter()                                                            # host round trip 2: the mutual matches
        mm = torch.nonzero(st['mutual'])                                                    # (pair, s) ascending; sizes its output
        pair_of, s_mid = mm[:, 0], mm[:, 1]
        t_mid = s_nn[pair_of, s_mid]
        m_counts = torch.bincount(pair_of, minlength=B).cpu().numpy()                       # matches per pair
        self.host_wait_s += time.perf_counter() - t0
        src_row = (2 * pair_of) * P + s_mid
        tgt_row = (2 * pair_of + 1) * P + t_mid
        ind = self.inlier.gathered(emb['equi'], src_row, tgt_row)      # BUFFER.py:291-292 rows 1..ele_n-2, gathered in-kernel
        ss_all, tt_all = kp[src_row].contiguous(), kp[tgt_row].contiguous()
        sR_all, tR_all = emb['R'][src_row].contiguous(), emb['R'][tgt_row].contiguous()
        # hypotheses, all-vs-all scoring, RANSAC and refinement of all B pairs: one set of launches (csrc/registration.hip,
        # batched section), bit-identical to the chain of single-pair calls (tests/pair_chain.py)
        all_poses = ops.recover_poses_batched(ind, ss_all, tt_all, sR_all, tR_all, m_counts, seeds, cfg)
        poses = [all_poses[b] for b in range(B)]
        if 'detail' in st:
            st['detail'].update(s_mids=s_mid, t_mids=t_mid, ind=ind, rows=(ss_all, tt_all, sR_all, tR_all))
        met = st.get('metrics')
        if met is None:
            return poses
        counts = ops.match_metrics(kp, s_nn, st['t_nn'], met['gt'], all_poses, met['tau_kp'], met['tau_match'], met['dist_th'])
        lost = np.nonzero(m_counts < 3)[0]                  # answered with the identity: never reached pose recovery
        if lost.size:
            counts[torch.from_numpy(lost).to(dev)] = -1
        return poses, counts

    def _metric_args(self, gt, tau_kp, tau_match, dist_th, B=1):
        """ground truth [B,4,4] (list of 4x4 / array / tensor, host or device) as f64 on the device + the three thresholds"""
        if isinstance(gt, (list, tuple)):
            gt = np.stack([g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g) for g in gt]).astype(np.float64) \
                if len(gt) else np.zeros((0, 4, 4))
        gt = torch.as_tensor(gt).to(self.device, torch.float64)
        if tuple(gt.shape) != (B, 4, 4):
            raise ValueError(f'metrics_gt: expected {B} ground-truth 4x4 poses, got shape {tuple(gt.shape)}')
        d = float(self.cfg.dist_th)
        return dict(gt=gt.contiguous(), tau_kp=d if tau_kp is None else float(tau_kp), tau_match=d if tau_match is None else float(tau_match),
                    dist_th=d if dist_th is None else float(dist_th))

    def _pair_detail(self, st):
        """register(detail=True): the state the stages left for a batch of ONE pair, in the per-cloud layout the parity tests and
        bench.py read.  pyr, axis, eps, score: the stacked pair; kpts, kaxis: two [P,3]; desc: two dicts of [P,...] slices of
        embed_patches (desc, equi, R, rand_axis, x, patches); s_mids, t_mids (int64, ascending s_mids), ind; inlier_num, best,
        inlier_mask, R_hyp, t_hyp from one hypotheses_score call on the pair's matched rows, the only launches detail adds (the
        batched recovery keeps these in its workspace; tests/test_pose_recovery_gpu.py pins the two equal)."""
        if 'detail' not in st:                              # a cloud without a keypoint: no stage was reached
            return {}
        cfg, P = self.cfg, self.cfg.num_keypts
        out = st['detail']
        out['kpts'], out['kaxis'] = ([st[k][i * P:(i + 1) * P] for i in range(2)] for k in ('kp', 'ka'))
        out['desc'] = [{k: (v[i * P:(i + 1) * P] if v is not None else None) for k, v in st['emb'].items()} for i in range(2)]
        rows = out.pop('rows')
        if out['ind'].shape[0] >= 3:
            R, t, num, best, mask = ops.hypotheses_score(out['ind'], *rows, cfg.azi_n, cfg.inlier_th)
            out.update(inlier_num=num, best=best, inlier_mask=mask, R_hyp=R, t_hyp=t)
        return out
