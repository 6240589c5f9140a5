"""The cost volume network on device (models/BUFFER.py:37-66,291-293).  Mutual matching and pose recovery (A12, A14-A16) are the
_describe / _match stages of pipeline.py over ops.knn and ops.recover_poses_batched."""
import numpy as np

from . import ops
from .patch_embedder import _fold_bn


class CostVolume:
    """CostVolume + CostNet (BUFFER.py:37-66, models/patchnet.py:88-147): one fused fp32-MFMA kernel
    (csrc/costnet.hip).  The kernel is written for the released geometry (32 channels, 5 elevation rows,
    azi_n = 20); anything else raises -- there is no library-convolution path in the product."""

    def __init__(self, W, device, azi_n=20, arith='f32', f24=None, f24b=None):
        if arith not in ('f32', 'split'):
            raise ValueError(f"cnn_arith must be 'f32' or 'split', got {arith!r}")
        if azi_n != 20:
            raise NotImplementedError(f'CostVolume: the fused kernel is built for azi_n = 20 (got {azi_n})')
        self.azi_n = azi_n
        p = 'Inlier.conv.ops'
        layers = []
        for i, bn in ((0, 1), (3, 4), (6, 7), (9, 10), (12, 13), (15, 16), (18, 19), (21, 22), (24, 25)):
            layers.append(_fold_bn(W[f'{p}.{i}.weight'], W[f'{p}.{i}.bias'], W[f'{p}.{bn}.running_mean'], W[f'{p}.{bn}.running_var']))
        layers.append((np.asarray(W[f'{p}.27.weight'], np.float32), np.asarray(W[f'{p}.27.bias'], np.float32)))
        # 'split': csrc/costnet_h3.hip -- the same network on the f16 matrix pipe, operands split hi + 2^-11 lo' (fp32-equivalent)
        # f24: the parts of the fp32 kernel (and of the split form's fp32 re-run) in the forms of csrc/costnet_w24.hip: 'all' | 'l2' | 'l4' | 'l6' | 'off'
        # (None: ops.COST_F24_DEFAULT)
        # f24b: the parts in the forms of csrc/costnet_w24b.hip beside them: 'all' | 'l1' | 'l3' | 'off' (None: ops.COST_F24B_DEFAULT when f24 is left
        # alone too, 'off' beside an explicit f24)
        cls = ops.CostVolumeNetSplit if arith == 'split' else ops.CostVolumeNet
        self.fused = cls(layers, device, f24=f24, f24b=f24b)

    def __call__(self, d1, d2):
        """d1,d2 f32[M,32,5,20] -> expected azimuth shift f32[M]."""
        if tuple(d1.shape[1:]) != (32, 5, 20) or d1.shape != d2.shape:
            raise ValueError(f'CostVolume: expected two [M,32,5,20] maps, got {tuple(d1.shape)} and {tuple(d2.shape)}')
        return self.fused(d1, d2)

    def gathered(self, equi, s_rows, t_rows):
        """full maps equi f32[rows,32,7,20] + matched row ids -> expected azimuth shift f32[M] (gather and elevation slice fused)."""
        return self.fused.gathered(equi, s_rows, t_rows)
