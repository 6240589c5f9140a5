"""Maximum-clique inlier selection with truncated-least-squares pose estimation on given correspondences, batched: the method made
known by TEASER++ (Yang, Shi, Carlone, T-RO 2021), the fourth pose estimator of the classical row beside the 3-point RANSAC, Fast
Global Registration and SC2-PCR -- the one that still works at a few per cent of true correspondences, and the only one that says
how trustworthy its consensus set is: no clique of the compatibility graph is larger than `bound` (largest core number + 1), so a
clique that reaches the bound is provably the largest consistent set (`certified`).  No TEASER++ source was at hand: the method is
restated from its published form (include/buffer_hip.h, N10; csrc/clique.hip; parity unpinned).  Deviations: scale fixed to 1, a
deterministic greedy clique instead of exact branch and bound, no certification stage, SC2's inlier refit appended.

    CliqueOptions         the estimator's parameters, their defaults, and their mapping onto the kernel
    clique_registration   any number of pairs with any correspondence lists in ONE ops.clique_batched call; no sampler and no seeds,
                          nothing read back
"""
from . import ops


class CliqueOptions:
    """d_thr: two correspondences are compatible when the distances between their source and their target points differ by at most
    d_thr; tim_thr: the truncation of the rotation's least squares over differences of correspondences (default: d_thr); t_thr: of the
    translation's per-axis vote (default: d_thr / 2); inlier_thr: residual below which a row counts in the refit (default: d_thr);
    max_seeds: greedy walks started, from the rows of largest core number; max_members: clique members that enter the pose;
    gnc_factor, gnc_iterations: the graduated non-convexity schedule; refine_iterations: most refits over the inliers."""

    def __init__(self, d_thr=0.1, tim_thr=None, t_thr=None, inlier_thr=None, max_seeds=64, max_members=256, gnc_factor=1.4,
                 gnc_iterations=100, refine_iterations=20):
        self.d_thr = float(d_thr)
        self.tim_thr = float(d_thr if tim_thr is None else tim_thr)
        self.t_thr = float(self.d_thr / 2 if t_thr is None else t_thr)
        self.inlier_thr = float(d_thr if inlier_thr is None else inlier_thr)
        self.max_seeds, self.max_members = int(max_seeds), int(max_members)
        self.gnc_factor, self.gnc_iterations, self.refine_iterations = float(gnc_factor), int(gnc_iterations), int(refine_iterations)

    def kernel_arguments(self):
        """-> the keyword arguments of ops.clique_batched"""
        return dict(d_thr=self.d_thr, tim_thr=self.tim_thr, t_thr=self.t_thr, inlier_thr=self.inlier_thr, max_seeds=self.max_seeds,
                    max_members=self.max_members, gnc_factor=self.gnc_factor, gnc_iterations=self.gnc_iterations,
                    refine_iterations=self.refine_iterations)

    def __repr__(self):
        return ('CliqueOptions(' + ', '.join(f'{k}={v!r}' for k, v in sorted(vars(self).items())) + ')')


def clique_registration(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, return_detail=False, **options):
    """src f32[sum src_lengths,3], tgt f32[sum tgt_lengths,3], corr int32[sum corr_lengths,2] (device; pair b owns the next lengths[b]
    rows of each, corr rows = (src row, tgt row) inside the pair's clouds), options = CliqueOptions' arguments
    -> dict(poses f64[B,4,4] src -> tgt, status int32[B] (index into ops.CLIQUE_STATUS), live int32[B], bound int32[B] (no consistent
    set is larger), clique int32[B] (the size found), certified bool[B] (clique == bound and status OK: the set is provably the
    largest), members_used int32[B], gnc_steps int32[B], inliers int32[B] (of the returned pose)), all on the device; with
    return_detail=True also winner_rank int32[B] and ops.clique_batched's detail arrays (deg, core, rank, sizes, members, weights,
    pose0, inlier_mask)."""
    opt = options.pop('options', None)
    if opt is None:
        opt = CliqueOptions(**options)
    elif options:
        raise TypeError('clique_registration: pass either options=CliqueOptions(...) or its arguments, not both')
    T, info, detail = ops.clique_batched(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, return_detail=return_detail,
                                         **opt.kernel_arguments())
    out = dict(poses=T, status=info[:, 0], live=info[:, 1], bound=info[:, 2], clique=info[:, 3],
               certified=(info[:, 3] == info[:, 2]) & (info[:, 0] == 1), members_used=info[:, 5], gnc_steps=info[:, 6],
               inliers=info[:, 7])
    if return_detail:
        out.update(winner_rank=info[:, 4], **detail)
    return out
