"""ICP on the device: the open3d `registration_icp` call that refines KITTI's odometry ground truth (KITTI/dataset.py:95-117:
point-to-point, threshold 0.20 m, identity init, <= 200 iterations, relative fitness / RMSE 1e-6), its point-to-plane form and
Generalized ICP (plane-to-plane, Segal et al.; open3d's registration_generalized_icp).

Per iteration: nearest target point inside the correspondence distance for every transformed source point (A2 cell grid:
column 0 of the distance-sorted neighbour row of csrc/radius.hip), fitness = matched / source points,
RMSE over the matches, then the update from the matches -- point-to-point: the rigid transform of the centred 3x3
cross-covariance in fp64, SVD with the det correction; point-to-plane: open3d's 6x6 step; generalized: the 6x6 Gauss-Newton step of
sum d^T (C(n_q) + R C(n_s) R^T)^-1 d with C(n) = I - (1 - epsilon) n n^T (include/buffer_hip.h, N2) -- composed onto the running
transform.
open3d's loop, restated; open3d itself is absent here (parity unpinned).

icp_batched runs that loop for many pairs at once in csrc/icp.hip (buf_icp_batched): state, correspondences, sums and updates
stay on the device; one int is read back every 8 rounds.  icp_point_to_point / icp_point_to_plane / icp_generalized are its one-pair
forms.

voxel_map / vgicp_batched / icp_voxelized: voxelized Generalized ICP (Koide et al. 2021; csrc/vgicp.hip, include/buffer_hip.h N9)
against a reusable map of target voxels, without a nearest-neighbour search."""
import numpy as np
import torch

from . import ops


def icp_batched(srcs, tgts, max_dist, inits=None, method='point_to_point', tgt_normals=None, max_iteration=30,
                relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False, src_normals=None, epsilon=1e-3):
    """ICP of B pairs in one set of launches (csrc/icp.hip, buf_icp_batched): srcs / tgts lists of f32[n_b,3] / f32[m_b,3]
    device tensors, inits None or B 4x4 transforms, method 'point_to_point' (Kabsch step),
    'point_to_plane' (open3d's step, restated, unpinned; needs tgt_normals, a list of f32[m_b,3]) or 'generalized' (plane-to-plane;
    needs tgt_normals and src_normals, a list of f32[n_b,3]; epsilon in (0, 1] is the covariance along a normal; a normal row that is
    not a unit vector counts as no normal, C = I).
    -> list of B dicts: T (f64[4,4] numpy src->tgt), fitness, inlier_rmse, iterations, and correspondences (int32[k,2] numpy,
    pair-local (source row, target row), only with return_correspondences).  Each pair's result does not depend on the
    others of the batch; one small readback per 8 rounds."""
    B = len(srcs)
    if len(tgts) != B:
        raise ValueError(f"icp_batched: {B} sources but {len(tgts)} targets")
    if inits is not None and len(inits) != B:
        raise ValueError(f"icp_batched: {B} pairs but {len(inits)} initial transforms")
    if method not in ops.ICP_METHODS:
        raise ValueError(f"icp_batched: unknown method {method!r} (one of {sorted(ops.ICP_METHODS)})")
    if method == 'point_to_plane':
        if tgt_normals is None:
            raise ValueError("icp_batched: point_to_plane needs tgt_normals (one f32[m,3] per target)")
        if len(tgt_normals) != B or any(tuple(n.shape) != tuple(t.shape) for n, t in zip(tgt_normals, tgts)):
            raise ValueError("icp_batched: tgt_normals must hold one [m,3] array per target, shaped like the target")
    if method == 'generalized':
        if src_normals is None or tgt_normals is None:
            raise ValueError("icp_batched: generalized needs src_normals and tgt_normals (one f32[n,3] per cloud)")
        for nrm, clouds, what in ((src_normals, srcs, 'src_normals'), (tgt_normals, tgts, 'tgt_normals')):
            if len(nrm) != B or any(tuple(n.shape) != tuple(c.shape) for n, c in zip(nrm, clouds)):
                raise ValueError(f"icp_batched: {what} must hold one [n,3] array per cloud, shaped like the cloud")
        if not (0.0 < float(epsilon) <= 1.0):
            raise ValueError(f"icp_batched: epsilon={epsilon} (must be in (0, 1])")
    if B == 0:
        return []
    if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in list(srcs) + list(tgts)):
        raise RuntimeError("icp_batched: expected tensors in device memory (buffer_amd has no CPU path)")
    dev = srcs[0].device
    src = torch.cat([s.reshape(-1, 3).float() for s in srcs])
    tgt = torch.cat([t.reshape(-1, 3).float() for t in tgts])
    nrm = torch.cat([n.reshape(-1, 3).float() for n in tgt_normals]) if method != 'point_to_point' else None
    snrm = torch.cat([n.reshape(-1, 3).float() for n in src_normals]) if method == 'generalized' else None
    sl = np.array([s.shape[0] for s in srcs], np.int32)
    tl = np.array([t.shape[0] for t in tgts], np.int32)
    T0 = np.stack([np.eye(4) if inits is None else np.asarray(inits[b], np.float64).reshape(4, 4) for b in range(B)])
    T, fit, rmse, iters, nn = ops.icp_batched(src, sl, tgt, tl, max_dist, torch.from_numpy(T0).to(dev), method, nrm, max_iteration,
                                              relative_fitness, relative_rmse, correspondences=return_correspondences,
                                              src_normals=snrm, epsilon=epsilon)
    T, fit, rmse, iters = T.cpu().numpy(), fit.cpu().numpy(), rmse.cpu().numpy(), iters.cpu().numpy()
    nn = nn.cpu().numpy() if nn is not None else None
    s_off, t_off = np.concatenate([[0], np.cumsum(sl)]), np.concatenate([[0], np.cumsum(tl)])
    out = []
    for b in range(B):
        r = dict(T=T[b], fitness=float(fit[b]), inlier_rmse=float(rmse[b]), iterations=int(iters[b]))
        if return_correspondences:
            row = nn[s_off[b]:s_off[b + 1]]
            hit = np.flatnonzero(row < t_off[-1])
            r['correspondences'] = np.stack([hit, row[hit] - t_off[b]], 1).astype(np.int32) if hit.size else np.zeros((0, 2), np.int32)
        out.append(r)
    return out


def _one_pair(src, tgt, max_dist, init, method, tgt_normals, max_iteration, relative_fitness, relative_rmse, src_normals=None,
              epsilon=1e-3):
    """icp_batched with one pair -> (T f64[4,4] numpy src->tgt, fitness, inlier_rmse, corr int32[k,2] numpy)."""
    if not (isinstance(src, torch.Tensor) and isinstance(tgt, torch.Tensor) and src.is_cuda and tgt.is_cuda):
        raise RuntimeError("icp: expected tensors in device memory (buffer_amd has no CPU path)")
    if tgt.shape[0] == 0:                                   # nothing to match: the initial transform, as open3d returns it
        return (np.eye(4) if init is None else np.asarray(init, np.float64).copy()), 0.0, 0.0, np.zeros((0, 2), np.int32)
    r = icp_batched([src], [tgt], max_dist, None if init is None else [init], method,
                    None if tgt_normals is None else [tgt_normals], max_iteration, relative_fitness, relative_rmse,
                    return_correspondences=True, src_normals=None if src_normals is None else [src_normals], epsilon=epsilon)[0]
    return r['T'], r['fitness'], r['inlier_rmse'], r['correspondences']


def icp_point_to_point(src, tgt, max_dist, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """src f32[n,3], tgt f32[m,3] (device) -> (T f64[4,4] numpy src->tgt, fitness, inlier_rmse, corr int32[k,2] numpy):
    icp_batched with one pair."""
    return _one_pair(src, tgt, max_dist, init, 'point_to_point', None, max_iteration, relative_fitness, relative_rmse)


def icp_point_to_plane(src, tgt, tgt_normals, max_dist, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """src f32[n,3], tgt / tgt_normals f32[m,3] (device) -> icp_point_to_point's return shape, point-to-plane step."""
    return _one_pair(src, tgt, max_dist, init, 'point_to_plane', tgt_normals, max_iteration, relative_fitness, relative_rmse)


def icp_generalized(src, src_normals, tgt, tgt_normals, max_dist, init=None, max_iteration=30, relative_fitness=1e-6,
                    relative_rmse=1e-6, epsilon=1e-3):
    """src / src_normals f32[n,3], tgt / tgt_normals f32[m,3] (device) -> icp_point_to_point's return shape, Generalized ICP step."""
    if not (0.0 < float(epsilon) <= 1.0):
        raise ValueError(f"icp_generalized: epsilon={epsilon} (must be in (0, 1])")
    return _one_pair(src, tgt, max_dist, init, 'generalized', tgt_normals, max_iteration, relative_fitness, relative_rmse, src_normals,
                     epsilon)


# ---------------------------------------------------------------------------------------------------- voxelized Generalized ICP (N9)
def _check_voxel(fn, voxel, epsilon):
    if voxel is None or not (0.0 < float(voxel) < float('inf')):
        raise ValueError(f"{fn}: voxel={voxel} (must be finite and > 0)")
    if not (0.0 < float(epsilon) <= 1.0):
        raise ValueError(f"{fn}: epsilon={epsilon} (must be in (0, 1])")


def _check_normals(fn, what, nrm, clouds):
    if nrm is not None and (len(nrm) != len(clouds) or any(tuple(n.shape) != tuple(c.shape) for n, c in zip(nrm, clouds))):
        raise ValueError(f"{fn}: {what} must hold one [n,3] array per cloud, shaped like the cloud")


def voxel_map(tgts, voxel, tgt_normals=None, epsilon=1e-3):
    """The voxel map of a list of target clouds f32[m_c,3] (device; tgt_normals None or one f32[m_c,3] per cloud) -> ops.VoxelMap: per
    occupied voxel of edge `voxel` a count, a mean and the mean of the points' covariances C(n) = I - (1 - epsilon) n n^T (C = I without
    a usable normal).  Built once, it serves any number of vgicp_batched calls and any number of pairs per cloud.  The voxel size
    trades accuracy for reach: a source point only meets the voxels at and beside the one it falls into."""
    _check_voxel("voxel_map", voxel, epsilon)
    if len(tgts) == 0:
        raise ValueError("voxel_map: no target cloud")
    _check_normals("voxel_map", "tgt_normals", tgt_normals, tgts)
    if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in tgts):
        raise RuntimeError("voxel_map: expected tensors in device memory (buffer_amd has no CPU path)")
    tgt = torch.cat([t.reshape(-1, 3).float() for t in tgts])
    nrm = torch.cat([n.reshape(-1, 3).float() for n in tgt_normals]) if tgt_normals is not None else None
    return ops.voxel_map_build(tgt, [t.shape[0] for t in tgts], float(voxel), nrm, float(epsilon))


def vgicp_batched(srcs, targets, inits=None, src_normals=None, tgt_normals=None, voxel=None, epsilon=1e-3, neighbors=7, pair_target=None,
                  max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, return_rows=False):
    """Voxelized Generalized ICP (Koide et al. 2021; csrc/vgicp.hip, include/buffer_hip.h N9) of B sources in one set of launches.
    targets: an ops.VoxelMap (voxel_map(), reused as often as wanted), or a list of clouds from which one is built with voxel=,
    tgt_normals and epsilon.  pair_target: None (pair b meets map cloud b) or B cloud indices; several pairs may share a cloud.
    neighbors: 1, 7 (default: the voxel and its six face neighbours) or 27.  src_normals: None (C = I) or one f32[n_b,3] per source.
    A source point meets every occupied voxel among the neighbours: no nearest-neighbour search and no distance threshold.
    -> icp_batched's list of dicts: T, fitness (source points that met a voxel / source points), inlier_rmse (root mean square
    distance to the VOXEL MEANS over all terms: of the order of the voxel size, not a surface residual, comparable only at equal voxel
    and neighbors), iterations, and with return_rows rows (int32[n_b]: the cloud-local map row of the voxel each point fell into, -1)."""
    B = len(srcs)
    if neighbors not in ops.VGICP_NEIGHBORS:
        raise ValueError(f"vgicp_batched: neighbors={neighbors} (one of {ops.VGICP_NEIGHBORS})")
    if inits is not None and len(inits) != B:
        raise ValueError(f"vgicp_batched: {B} pairs but {len(inits)} initial transforms")
    _check_normals("vgicp_batched", "src_normals", src_normals, srcs)
    is_map = isinstance(targets, ops.VoxelMap)
    if is_map:
        if voxel is not None or tgt_normals is not None:
            raise ValueError("vgicp_batched: voxel / tgt_normals belong to the map that was built, not to a call on it")
        nclouds = targets.nclouds
    else:
        _check_voxel("vgicp_batched", voxel, epsilon)
        _check_normals("vgicp_batched", "tgt_normals", tgt_normals, targets)
        nclouds = len(targets)
    if pair_target is None:
        if B != nclouds:
            raise ValueError(f"vgicp_batched: {B} sources but {nclouds} targets (name each pair's target with pair_target)")
    else:
        pair_target = [int(c) for c in pair_target]
        if len(pair_target) != B or any(c < 0 or c >= nclouds for c in pair_target):
            raise ValueError(f"vgicp_batched: pair_target must hold {B} indices into the {nclouds} targets")
    if B == 0:
        return []
    if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in srcs):
        raise RuntimeError("vgicp_batched: expected tensors in device memory (buffer_amd has no CPU path)")
    vmap = targets if is_map else voxel_map(targets, voxel, tgt_normals, epsilon)
    dev = srcs[0].device
    src = torch.cat([s.reshape(-1, 3).float() for s in srcs])
    snrm = torch.cat([n.reshape(-1, 3).float() for n in src_normals]) if src_normals is not None else None
    sl = np.array([s.shape[0] for s in srcs], np.int32)
    T0 = np.stack([np.eye(4) if inits is None else np.asarray(inits[b], np.float64).reshape(4, 4) for b in range(B)])
    T, fit, rmse, iters, row = ops.vgicp_batched(src, sl, vmap, torch.from_numpy(T0).to(dev), neighbors, snrm, pair_target, max_iteration,
                                                 relative_fitness, relative_rmse, rows=return_rows)
    T, fit, rmse, iters = T.cpu().numpy(), fit.cpu().numpy(), rmse.cpu().numpy(), iters.cpu().numpy()
    row = row.cpu().numpy() if row is not None else None
    s_off = np.concatenate([[0], np.cumsum(sl)])
    out = []
    for b in range(B):
        r = dict(T=T[b], fitness=float(fit[b]), inlier_rmse=float(rmse[b]), iterations=int(iters[b]))
        if return_rows:
            r['rows'] = row[s_off[b]:s_off[b + 1]].copy()
        out.append(r)
    return out


def icp_voxelized(src, src_normals, tgt, tgt_normals, voxel, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                  epsilon=1e-3, neighbors=7):
    """The one-pair form of vgicp_batched: src / tgt f32[n,3] / f32[m,3] (device), normals like them or None
    -> (T f64[4,4] numpy src->tgt, fitness, inlier_rmse, rows int32[n] numpy)."""
    _check_voxel("icp_voxelized", voxel, epsilon)
    r = vgicp_batched([src], [tgt], None if init is None else [init], None if src_normals is None else [src_normals],
                      None if tgt_normals is None else [tgt_normals], voxel, epsilon, neighbors, None, max_iteration, relative_fitness,
                      relative_rmse, return_rows=True)[0]
    return r['T'], r['fitness'], r['inlier_rmse'], r['rows']
