"""SC2-PCR (Chen, Sun, Yang, Tao, CVPR 2022: second order spatial compatibility) on given correspondences, batched: the third pose
estimator of the classical row beside the 3-point RANSAC and Fast Global Registration -- a deterministic consensus estimator for low
inlier ratios, where both of those break down.  The single-stage form: the paper's second sampling stage and its learned variants are
not provided.  No SC2-PCR source was at hand: the algorithm is restated from its published form (include/buffer_hip.h, N8;
csrc/sc2.hip; parity with any other implementation unpinned).

    Sc2Options         the estimator's parameters, their defaults, and their mapping onto the kernel
    sc2_registration   any number of pairs with any correspondence lists (FPFH matches, the learned path's mutual matches) in ONE
                       ops.sc2_batched call; no sampler and no seeds, nothing read back
"""
from . import ops


class Sc2Options:
    """d_thr: two correspondences are compatible when the distances between their source and their target points differ by at most
    d_thr; inlier_thr: residual below which a row counts for a pose (default: d_thr); seed_ratio, max_seeds: the share of the rows
    taken as seeds and its cap; k1: the size of a seed's consensus set; nms_radius: non-maximum suppression of the seeds among source
    points (0: none); power_iterations: of the leading-eigenvector iterations (global confidence and each set's weights);
    refine_iterations: most refits over the winner's inliers."""

    def __init__(self, d_thr=0.1, inlier_thr=None, seed_ratio=0.2, max_seeds=512, k1=30, nms_radius=0.0, power_iterations=10,
                 refine_iterations=20):
        self.d_thr, self.inlier_thr = float(d_thr), float(d_thr if inlier_thr is None else inlier_thr)
        self.seed_ratio, self.max_seeds, self.k1, self.nms_radius = float(seed_ratio), int(max_seeds), int(k1), float(nms_radius)
        self.power_iterations, self.refine_iterations = int(power_iterations), int(refine_iterations)

    def kernel_arguments(self):
        """-> the keyword arguments of ops.sc2_batched"""
        return dict(d_thr=self.d_thr, inlier_thr=self.inlier_thr, seed_ratio=self.seed_ratio, max_seeds=self.max_seeds, k1=self.k1,
                    nms_radius=self.nms_radius, power_iterations=self.power_iterations, refine_iterations=self.refine_iterations)

    def __repr__(self):
        return ('Sc2Options(' + ', '.join(f'{k}={v!r}' for k, v in sorted(vars(self).items())) + ')')


def sc2_registration(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, return_detail=False, **options):
    """src f32[sum src_lengths,3], tgt f32[sum tgt_lengths,3], corr int32[sum corr_lengths,2] (device; pair b owns the next lengths[b]
    rows of each, corr rows = (src row, tgt row) inside the pair's clouds), options = Sc2Options' arguments
    -> dict(poses f64[B,4,4] src -> tgt, status int32[B] (index into ops.SC2_STATUS), live int32[B], seeds int32[B], winner int32[B]
    (the winning seed's row, -1 without one), inliers int32[B] (of the returned pose)), all on the device; with return_detail=True also
    winner_count int32[B] (before refinement), confidence f64[sum n], seed_rows / hyp_counts int32[B,max_seeds], counts
    int32[max_seeds * sum n] and inlier_mask uint8[sum n] (ops.sc2_batched's detail)."""
    opt = options.pop('options', None)
    if opt is None:
        opt = Sc2Options(**options)
    elif options:
        raise TypeError('sc2_registration: pass either options=Sc2Options(...) or its arguments, not both')
    T, info, detail = ops.sc2_batched(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, return_detail=return_detail,
                                      **opt.kernel_arguments())
    out = dict(poses=T, status=info[:, 0], live=info[:, 1], seeds=info[:, 2], winner=info[:, 3], inliers=info[:, 5])
    if return_detail:
        out.update(winner_count=info[:, 4], confidence=detail['confidence'], seed_rows=detail['seeds'], hyp_counts=detail['hyp_counts'],
                   counts=detail['counts'], inlier_mask=detail['inlier_mask'])
    return out
