"""The independent pair-by-pair registration chain (test infrastructure): what BufferPipeline's stacked path is held against with
torch.equal.  One pair at a time, a compaction per cloud, the mutual check on one pair's 1-NN rows, the dense cost net on gathered and
sliced maps, and the three single-pair pose-recovery calls -- none of the stacked batch's indexing, the gather form of the cost net or
buf_recover_poses_batched.  Written against public pieces of buffer_amd only."""
import torch

from buffer_amd import ops, pyramid
from buffer_amd.point_learner import orient_axes


def mutual_matching(src_des, tgt_des):
    """buffer.mutual_matching (BUFFER.py:335-359): 1-NN both ways (csrc/pointops.hip k_knn), mutual check.
    -> (s_mids, t_mids) int64 device tensors (ascending s_mids, as np.where yields them)."""
    _, s_idx = ops.knn(tgt_des[None], src_des[None], 1)
    _, t_idx = ops.knn(src_des[None], tgt_des[None], 1)
    s_nn, t_nn = s_idx[0, :, 0], t_idx[0, :, 0]
    ar = torch.arange(s_nn.shape[0], device=s_nn.device)
    s_mids = torch.nonzero(t_nn[s_nn] == ar).flatten()
    return s_mids, s_nn[s_mids]


def recover_pose(ind, ss_kpts, tt_kpts, ss_R, tt_R, cfg, seed=0):
    """BUFFER.py:295-333: hypotheses, all-vs-all scoring, RANSAC on the winner's inliers, refinement -> pose f32[4,4] device."""
    R, t, num, best, mask = ops.hypotheses_score(ind, ss_kpts, tt_kpts, ss_R, tt_R, cfg.azi_n, cfg.inlier_th)
    T, info = ops.ransac_kabsch_masked(ss_kpts, tt_kpts, mask, cfg.ransac_hypotheses, seed, cfg.dist_th, cfg.similar_th)
    if cfg.pose_refine:
        T, _ = ops.post_refine(T, ss_kpts, tt_kpts, cfg.refine_threshold, 20)
    return T


@torch.no_grad()
def register(pipe, inp, seed=0, perms=None):
    """inp from pipe.upload() -> pose f32[4,4] (src -> tgt) with pipe's networks, limits and configuration; the identity for a pair with
    a cloud that has no keypoint or with fewer than 3 mutual matches (ThreeDMatch/test.py:242-245)."""
    cfg = pipe.cfg
    identity = torch.eye(4, device=pipe.device)
    pyr = pyramid.build_pyramid(inp['points'], inp['lengths'], pipe.limits, cfg)
    n_src = int(inp['lengths'][0])
    axis, eps, bottle, skips, _ = pipe.point.efcnn(pyr, inp['features'])
    score = pipe.point.detnet(pyr, bottle, skips)
    pts0 = pyr['points'][0]
    cand_p, cand_a = [], []
    for lo, hi in ((0, n_src), (n_src, pts0.shape[0])):
        p = pts0[lo:hi]
        a = orient_axes(axis[lo:hi], p)
        keep = ops.compact_greater(score[lo:hi, 0], cfg.keypts_th).long()       # BUFFER.py:255-259
        if keep.shape[0] == 0:
            return identity
        cand_p.append(p[keep]); cand_a.append(a[keep])
    # both fragments sampled in one launch, one workgroup per cloud (BUFFER.py:266-271)
    fps = ops.furthest_point_sample_ragged(torch.cat(cand_p), [c.shape[0] for c in cand_p], cfg.num_keypts).long()
    kp = [cand_p[i][fps[i]].contiguous() for i in range(2)]
    ka = [cand_a[i][fps[i]].contiguous() for i in range(2)]
    raws = (inp['src_raw'], inp['tgt_raw'])
    if perms is not None:                               # caller-pinned permutations
        sup = torch.cat([raws[i][perms[i]] for i in range(2)]).contiguous()
        sup_len = [raws[0].shape[0], raws[1].shape[0]]
    else:                                               # keyed device permutation, the same one register_batch uses
        sup, sup_len = ops.permute_clouds(raws, [ops.perm_key(seed, j) for j in range(2)])
    P = cfg.num_keypts
    patches = ops.select_patches_batched(sup, sup_len, torch.cat(kp), P, cfg.des_r, cfg.num_points_per_patch)
    emb = pipe.desc.embed_patches(patches, torch.cat(ka))
    res = [{k: (v[i * P:(i + 1) * P] if v is not None else None) for k, v in emb.items()} for i in range(2)]
    s_mids, t_mids = mutual_matching(res[0]['desc'], res[1]['desc'])
    if s_mids.shape[0] < 3:
        return identity
    ss_kpts, tt_kpts = kp[0][s_mids].contiguous(), kp[1][t_mids].contiguous()
    e = cfg.ele_n
    ind = pipe.inlier(res[0]['equi'][s_mids][:, :, 1:e - 1].contiguous(), res[1]['equi'][t_mids][:, :, 1:e - 1].contiguous())
    return recover_pose(ind, ss_kpts, tt_kpts, res[0]['R'][s_mids].contiguous(), res[1]['R'][t_mids].contiguous(), cfg, seed)
