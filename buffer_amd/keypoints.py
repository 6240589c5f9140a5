"""Classical keypoint detection: Intrinsic Shape Signatures (Zhong 2009, in the simplified form of open3d's compute_iss_keypoints;
csrc/iss.hip, buf_iss_keypoints; restated from the published form, parity unpinned: include/buffer_hip.h N11 is the specification).

    iss_keypoints       keypoints of one or several stacked clouds: one cell grid, two radius queries, one launch pair, one compaction
"""
import numpy as np
import torch

from . import ops


def _whole_row_k(grid, points, lens, radii):
    """the longest row of each radius (count-only queries; both maxima come back in one read)"""
    mc = torch.zeros(len(radii), dtype=torch.int32, device=points.device)
    for c, r in enumerate(radii):
        grid.query(points, lens, 0, radius=r, max_count=mc[c:c + 1])
    return [max(int(v), 1) for v in mc.tolist()]


def iss_keypoints(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, lengths=None, max_nn=None,
                  return_saliency=False, grid=None):
    """points f32[n,3] (device; several clouds stacked when `lengths` int[nc] is given) -> (idx int64[K] on the device: the global rows
    of the keypoints, ascending; counts int64[nc] on the host: keypoints per cloud) and with return_saliency also saliency f64[n] and
    the eigenvalues f64[n,3] (descending) of every point.
    A point is a keypoint when the eigenvalues l1 >= l2 >= l3 of the covariance of its neighbours inside salient_radius (itself
    included, at least min_neighbors of them) satisfy l2 < gamma_21 l1 and l3 < gamma_32 l2, and no neighbour inside non_max_radius
    (at least min_neighbors again) has a larger l3.  Neighbours stay inside a point's cloud.
    One CellGrid over the stacked clouds at the larger radius (`grid`: one built elsewhere over the same points and lengths, with a
    radius no smaller), a count-only query per radius so that k holds the longest row (whole rows, as open3d's radius search gives;
    max_nn, when given, is k instead and keeps the nearest max_nn), the two row queries in the grid's order, one buf_iss_keypoints call,
    ops.compact_greater on the mask.  The compaction's count is the one read-back the host waits for (the per-cloud counts arrive with
    it); max_nn=None adds the read of the two row lengths."""
    points = ops._dev(points, torch.float32, "iss_keypoints.points")
    n = int(points.shape[0])
    lens = np.array([n], np.int32) if lengths is None else np.asarray(lengths, np.int32).reshape(-1)
    if int(lens.sum()) != n:
        raise ValueError(f"iss_keypoints: lengths sum to {int(lens.sum())}, points holds {n} rows")
    rs, rn = float(salient_radius), float(non_max_radius)
    if not (0.0 < rs < float('inf') and 0.0 < rn < float('inf')):
        raise ValueError(f"iss_keypoints: salient_radius={salient_radius}, non_max_radius={non_max_radius} (finite, > 0)")
    if max_nn is not None and int(max_nn) < 1:
        raise ValueError(f"iss_keypoints: max_nn={max_nn} (None or >= 1)")
    dev = points.device
    if n == 0:
        res = (torch.zeros(0, dtype=torch.int64, device=dev), np.zeros(len(lens), np.int64))
        return res + (torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros((0, 3), dtype=torch.float64, device=dev)) if return_saliency else res
    if grid is None:
        grid = ops.CellGrid(points, lens, max(rs, rn))
    elif grid.radius < max(rs, rn) or grid.ns != n or not np.array_equal(grid.s_lengths, lens):
        raise ValueError("iss_keypoints: the given grid does not cover these clouds at these radii")
    same = rs == rn
    if max_nn is None:
        ks, kn = _whole_row_k(grid, points, lens, [rs] if same else [rs, rn]) * (2 if same else 1)
    else:
        ks = kn = int(max_nn)
    nbr_sal = grid.query(points, lens, ks, radius=rs, q_order=grid.order)
    nbr_nms = nbr_sal if same else grid.query(points, lens, kn, radius=rn, q_order=grid.order)
    mask, sal, eig = ops.iss_keypoints(points, nbr_sal, nbr_nms, gamma_21, gamma_32, min_neighbors, 0, return_eig=return_saliency)
    # keypoints per cloud, formed on the device and copied behind the kernels: the compaction's read-back waits for the copy as well
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])).to(dev)
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(mask, 0, dtype=torch.int64)])
    counts_h = torch.empty(len(lens), dtype=torch.int64, pin_memory=True)
    counts_h.copy_(csum[off[1:]] - csum[off[:-1]], non_blocking=True)
    idx = ops.compact_greater(mask.float(), 0.5).long()
    torch.cuda.current_stream().synchronize()                   # (already drained by the compaction's read-back)
    counts = counts_h.numpy().copy()
    return (idx, counts, sal, eig) if return_saliency else (idx, counts)
