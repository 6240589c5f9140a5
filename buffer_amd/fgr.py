"""Fast Global Registration (Zhou, Park, Koltun 2016) on given correspondences, batched: the second pose estimator of the classical
row beside the 3-point RANSAC -- in open3d terms registration_fast_based_on_feature_matching after the matching.  open3d is absent
here: the algorithm is restated from its published form (include/buffer_hip.h, N7; csrc/fgr.hip; parity unpinned).

    FgrOptions                 open3d's FastGlobalRegistrationOption: its names and defaults, and their mapping onto the kernel's
    fast_global_registration   any number of pairs with any correspondence lists (FPFH matches, the learned path's mutual matches)
                               in ONE ops.fgr_batched call; deterministic given the seeds, nothing read back
"""
import sys

from . import ops


class FgrOptions:
    """division_factor: mu is divided by it; use_absolute_scale: measure in the clouds' own units (not provided: the clouds are always
    normalised); decrease_mu: anneal mu at all; maximum_correspondence_distance: where the annealing stops -- read in normalised
    units as open3d reads it, or with delta_absolute=True in the clouds' units as the paper states it; iteration_number; tuple_scale,
    maximum_tuple_count: the tuple test.  trial_factor, mu_start, decrease_every: open3d's constants 100, 1.0 and 4."""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, delta_absolute=False, trial_factor=100, mu_start=1.0,
                 decrease_every=4):
        self.division_factor, self.use_absolute_scale, self.decrease_mu = float(division_factor), bool(use_absolute_scale), bool(decrease_mu)
        self.maximum_correspondence_distance, self.iteration_number = float(maximum_correspondence_distance), int(iteration_number)
        self.tuple_scale, self.maximum_tuple_count = float(tuple_scale), int(maximum_tuple_count)
        self.delta_absolute, self.trial_factor, self.mu_start, self.decrease_every = bool(delta_absolute), int(trial_factor), float(mu_start), int(decrease_every)

    def kernel_arguments(self):
        """-> the keyword arguments of ops.fgr_batched"""
        if self.use_absolute_scale:
            raise NotImplementedError('FgrOptions: use_absolute_scale=True is not provided (the clouds are always normalised)')
        delta, absolute = self.maximum_correspondence_distance, self.delta_absolute
        if not self.decrease_mu:
            delta, absolute = sys.float_info.max, False           # a floor that mu never passes: it is never divided
        return dict(tuple_scale=self.tuple_scale, max_tuples=self.maximum_tuple_count, trial_factor=self.trial_factor,
                    mu_start=self.mu_start, delta=delta, delta_absolute=absolute, division_factor=self.division_factor,
                    decrease_every=self.decrease_every, iterations=self.iteration_number)

    def __repr__(self):
        return ('FgrOptions(' + ', '.join(f'{k}={v!r}' for k, v in sorted(vars(self).items())) + ')')


def fast_global_registration(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, seeds=None, return_rows=False, **options):
    """src f32[sum src_lengths,3], tgt f32[sum tgt_lengths,3], corr int32[sum corr_lengths,2] (device; pair b owns the next lengths[b]
    rows of each, corr rows = (src row, tgt row) inside the pair's clouds), seeds[b] (default b), options = FgrOptions' arguments
    -> dict(poses f64[B,4,4] src -> tgt, status int32[B] (index into ops.FGR_STATUS), tuples int32[B], trials int32[B], iterations
    int32[B] = updates applied), all on the device; with return_rows=True also rows int32[B,3*maximum_tuple_count,2] (the kept
    correspondences, tail -1) and weights f64[B,3*maximum_tuple_count] (their line-process weights, tail NaN)."""
    opt = options.pop('options', None)
    if opt is None:
        opt = FgrOptions(**options)
    elif options:
        raise TypeError('fast_global_registration: pass either options=FgrOptions(...) or its arguments, not both')
    T, info, rows, weights = ops.fgr_batched(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, seeds, return_rows=return_rows,
                                             **opt.kernel_arguments())
    out = dict(poses=T, status=info[:, 0], tuples=info[:, 1], trials=info[:, 2], iterations=info[:, 3])
    if return_rows:
        out.update(rows=rows, weights=weights)
    return out
