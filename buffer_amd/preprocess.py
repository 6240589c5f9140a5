"""N1 -- the open3d pre-processing of the reference's datasets on device
(ThreeDMatch/dataset.py:89-153, KITTI/dataset.py): `voxel_down_sample`, `estimate_normals` (30-NN),
`orient_normals_towards_camera_location`, behind csrc/preprocess.hip.  open3d (0.13.0, README.md:28) is absent from
/root/reference and from this image: parity unpinned, algorithms restated from its published sources."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .ops import _dev, _ptr, _stream


_SHUFFLE_SALT = 0x5851F42D4C957F2D


def voxel_down_sample(points, voxel_size, normals=None, max_cells=0):
    """open3d PointCloud.voxel_down_sample: points f32|f64[n,3] (device) -> f64[m,3] voxel means
    (, f64[m,3] mean normals), rows in ascending voxel-key order."""
    L = _lib.lib()
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _lib.BufferHipError("voxel_down_sample: expected a tensor in device memory (buffer_amd has no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.BufferHipError("voxel_down_sample: points.shape is not (N, 3)")
    if not voxel_size > 0:
        raise _lib.BufferHipError("voxel_down_sample: voxel_size <= 0.")          # open3d's message
    dt = torch.float64 if points.dtype == torch.float64 else torch.float32
    points = points.to(dt).contiguous()
    if normals is not None:
        normals = _dev(normals, dt, "voxel_down_sample.normals")
    n = int(points.shape[0])
    if max_cells <= 0:
        max_cells = max(1 << 16, 4 * n)          # bucket table of the counting sort: the result does not depend on it, the scan over it costs
    nbytes = L.buf_voxel_downsample_ws_bytes(n, max_cells)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=points.device)
    out_n = torch.empty((max(n, 1), 3), dtype=torch.float64, device=points.device) if normals is not None else None
    m = C.c_int(0)
    check(L.buf_voxel_downsample(_ptr(points), _ptr(normals), 1 if dt == torch.float64 else 0, n, float(voxel_size),
                                 _ptr(out), _ptr(out_n), C.byref(m), max_cells, _ptr(ws), nbytes, _stream()),
          "buf_voxel_downsample")
    if normals is not None:
        return out[:m.value], out_n[:m.value]
    return out[:m.value]


def voxel_down_sample_batch(points, lengths, voxel_size, max_cells=0):
    """voxel_down_sample for several clouds stacked in `points` (f32|f64[sum n_c,3], lengths int[nc]) in one set of launches and
    one host round trip -> (f64[sum m_c,3] voxel means cloud after cloud, int32[nc] row counts); cloud by cloud the rows are
    those of voxel_down_sample."""
    L = _lib.lib()
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _lib.BufferHipError("voxel_down_sample_batch: expected a tensor in device memory (buffer_amd has no CPU path)")
    if not voxel_size > 0:
        raise _lib.BufferHipError("voxel_down_sample: voxel_size <= 0.")
    dt = torch.float64 if points.dtype == torch.float64 else torch.float32
    points = points.to(dt).contiguous()
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    n, nb = int(points.shape[0]), int(lens.shape[0])
    if int(lens.sum()) != n or nb == 0:
        raise _lib.BufferHipError("voxel_down_sample_batch: lengths do not sum to the number of points")
    if max_cells <= 0:
        max_cells = max(1 << 16, 4 * n, 2 * nb)
    nbytes = L.buf_voxel_downsample_batch_ws_bytes(n, nb, max_cells)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=points.device)
    out_lens = np.zeros(nb, np.int32)
    check(L.buf_voxel_downsample_batch(_ptr(points), 1 if dt == torch.float64 else 0, n, lens.ctypes.data_as(C.c_void_p), nb,
                                       float(voxel_size), _ptr(out), out_lens.ctypes.data_as(C.c_void_p), max_cells, _ptr(ws), nbytes,
                                       _stream()), "buf_voxel_downsample_batch")
    return out[:int(out_lens.sum())], out_lens


def estimate_normals(points, knn=30, camera=(0.0, 0.0, 0.0), orient=True, radius=None, ncand=40, grow=1.35, lengths=None):
    """open3d estimate_normals(KDTreeSearchParamKNN(knn)) [+ orient_normals_towards_camera_location(camera)]:
    points f32[n,3] (device) -> unit normals f32[n,3].  `lengths` (optional): the rows are several clouds stacked
    (neighbours are searched inside a point's own cloud) -- one set of launches for all of them; the normals equal those of
    cloud-by-cloud calls (each point ends with its exact knn nearest neighbours either way).

    k-NN through the cell grid of the radius search: candidates = the `ncand` nearest inside a ball (fp32, sorted), re-ranked
    in fp64 by the kernel; rows whose ball held fewer than min(knn, n) points are retried with a `grow` times larger
    radius (small steps keep the balls under the 64 candidates the wave-per-query radius kernel handles in one pass)."""
    L = _lib.lib()
    pts = _dev(points, torch.float32, "estimate_normals")
    n = int(pts.shape[0])
    out = torch.zeros((n, 3), dtype=torch.float32, device=pts.device)
    if n == 0:
        return out
    lens = np.array([n], np.int32) if lengths is None else np.asarray(lengths, np.int32)
    if int(lens.sum()) != n:
        raise _lib.BufferHipError("estimate_normals: lengths do not sum to the number of points")
    if len(lens) > 1 and int(lens[lens > 0].min()) <= knn:       # a cloud smaller than the neighbourhood: one by one
        lo = 0
        for m in lens:
            out[lo:lo + m] = estimate_normals(pts[lo:lo + m], knn, camera, orient, radius, ncand, grow)
            lo += int(m)
        return out
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ncand = max(int(ncand), int(knn))
    if radius is None:
        # pilot: distance to the knn-th neighbour for a few hundred queries of the first cloud (plumbing; sets only the first radius)
        n0 = int(lens[0]) if int(lens[0]) > knn else n
        g = torch.Generator(device=pts.device).manual_seed(0)
        sel = torch.randperm(n0, generator=g, device=pts.device)[:256]
        d = torch.cdist(pts[:n0][sel].double(), pts[:n0].double())
        kth = torch.topk(d, min(int(knn), n0), dim=1, largest=False).values[:, -1]
        radius = float(kth.median().item()) * 1.1 + 1e-9
    cam = (C.c_double * 3)(*[float(c) for c in camera])
    todo = None
    q_lens = lens
    r = float(radius)
    for _ in range(200):
        grid = ops.CellGrid(pts, lens, r)
        q = pts if todo is None else pts[todo.long()].contiguous()
        nq = int(q.shape[0])
        cand = grid.query(q, q_lens, ncand)
        deficient = torch.empty((nq,), dtype=torch.uint8, device=pts.device)
        check(L.buf_knn_normals(_ptr(pts), n, _ptr(todo), nq, _ptr(cand), ncand, int(knn), cam, 1 if orient else 0,
                                _ptr(out), _ptr(deficient), _stream()), "buf_knn_normals")
        bad = torch.nonzero(deficient).reshape(-1).to(torch.int32)
        if bad.numel() == 0:
            return out
        todo = bad if todo is None else todo[bad.long()].contiguous()
        if len(lens) > 1:                                        # retried rows per cloud (ascending indices)
            t_host = todo.cpu().numpy()
            q_lens = np.diff(np.searchsorted(t_host, offs)).astype(np.int32)
        else:
            q_lens = np.array([todo.shape[0]], np.int32)
        r *= grow
    raise _lib.BufferHipError("estimate_normals: neighbourhood search did not converge")


def _radius_rows(fn, points, radius, max_nn, lengths, grid):
    """the rows of estimate_normals_radius / estimate_covariances -> (points, nbr int32[n,k] or None when n == 0, grid)"""
    pts = _dev(points, torch.float32, fn)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{fn}: points {tuple(pts.shape)} is not [N,3]")
    n = int(pts.shape[0])
    lens = np.array([n], np.int32) if lengths is None else np.asarray(lengths, np.int32).reshape(-1)
    if int(lens.sum()) != n:
        raise ValueError(f"{fn}: lengths sum to {int(lens.sum())}, points holds {n} rows")
    r = float(radius)
    if not (0.0 < r < float('inf')):
        raise ValueError(f"{fn}: radius={radius} (finite, > 0)")
    if max_nn is not None and int(max_nn) < 1:
        raise ValueError(f"{fn}: max_nn={max_nn} (None or >= 1)")
    if n == 0:
        return pts, None, grid
    if grid is None:
        grid = ops.CellGrid(pts, lens, r)
    elif grid.radius < r or grid.ns != n or not np.array_equal(grid.s_lengths, lens):
        raise ValueError(f"{fn}: the given grid does not cover these clouds at this radius")
    if max_nn is None:                                           # whole rows: k = the longest one (the call's one host wait)
        mc = torch.zeros(1, dtype=torch.int32, device=pts.device)
        grid.query(pts, lens, 0, radius=r, max_count=mc)
        k = max(int(mc.item()), 1)
    else:
        k = int(max_nn)
    return pts, grid.query(pts, lens, k, radius=r, q_order=grid.order), grid


def estimate_normals_radius(points, radius, max_nn=30, camera=(0.0, 0.0, 0.0), orient=True, lengths=None, grid=None, return_cov=False):
    """open3d estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) [+ orient_normals_towards_camera_location(camera)], and with
    max_nn=None KDTreeSearchParamRadius(radius): points f32[n,3] (device; several clouds stacked when `lengths` int[nc] is given)
    -> unit normals f32[n,3] (, covariances f64[n,6] = (c00, c01, c02, c11, c12, c22)).  The neighbours of a point are the max_nn
    nearest inside `radius` within its own cloud, itself included; fewer than 3 give (0, 0, 1) and the identity covariance.
    One CellGrid over the stacked clouds (grid: one built elsewhere over the same points and lengths with a radius no smaller, e.g.
    the one fpfh.compute_fpfh and keypoints.iss_keypoints use: the rows, and so the result, are the same), one query with k = max_nn
    in the grid's order, one buf_row_normals launch (include/buffer_hip.h N13): no retry and nothing read back.  max_nn=None adds a
    count-only query whose maximum, the longest row, is k: the call's single host wait.  The launch itself runs in input order: its
    `order` argument measured 2 to 8 % slower than none (the row reads, not the gathers, carry the kernel).  A given grid
    with a larger radius costs query time (2.5 x the radius: 2.2 x / 4.8 x the whole call): share one at a similar radius."""
    pts, nbr, grid = _radius_rows("estimate_normals_radius", points, radius, max_nn, lengths, grid)
    if nbr is None:
        out = torch.zeros((0, 3), dtype=torch.float32, device=pts.device)
        return (out, torch.zeros((0, 6), dtype=torch.float64, device=pts.device)) if return_cov else out
    return ops.row_normals(pts, nbr, 0, camera if orient else None, return_cov=return_cov)


def estimate_covariances(points, radius, max_nn=30, camera=(0.0, 0.0, 0.0), orient=True, lengths=None, grid=None):
    """open3d estimate_covariances(KDTreeSearchParamHybrid(radius, max_nn) | KDTreeSearchParamRadius(radius) with max_nn=None):
    the covariances f64[n,6] = (c00, c01, c02, c11, c12, c22) of estimate_normals_radius' neighbourhoods, by the same launch.  The
    arguments are estimate_normals_radius' (camera and orient are taken so that one argument list serves both; a covariance has no sign)."""
    pts, nbr, grid = _radius_rows("estimate_covariances", points, radius, max_nn, lengths, grid)
    if nbr is None:
        return torch.zeros((0, 6), dtype=torch.float64, device=pts.device)
    return ops.row_normals(pts, nbr, 0, None, return_cov=True)[1]


def _stacked(fn, points, lengths):
    """points f32[n,3] on the device and the host lengths of the stacked clouds (one cloud without `lengths`)"""
    pts = _dev(points, torch.float32, fn)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{fn}: points {tuple(pts.shape)} is not [N,3]")
    n = int(pts.shape[0])
    lens = np.array([n], np.int32) if lengths is None else np.asarray(lengths, np.int32).reshape(-1)
    if lens.shape[0] < 1 or (lens < 0).any() or int(lens.sum()) != n:
        raise ValueError(f"{fn}: lengths sum to {int(lens.sum())}, points holds {n} rows")
    return pts, lens


def _knn_pilot_cell(pts, lens, k):
    """Cell edge for a k-NN search: the median distance to the k-th neighbour over a few hundred sampled points of the largest cloud
    (the pilot of estimate_normals; plumbing, it sets the grid's cell edge and so the speed, never the result)."""
    b = int(np.argmax(lens))
    lo, n0 = int(lens[:b].sum()), int(lens[b])
    if n0 < 2:
        return 1.0
    g = torch.Generator(device=pts.device).manual_seed(0)
    sel = torch.randperm(n0, generator=g, device=pts.device)[:256]
    cloud = pts[lo:lo + n0].double()
    d = torch.cdist(cloud[sel], cloud)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    kth = torch.topk(d, min(int(k), n0), dim=1, largest=False).values[:, -1]
    kth = kth[torch.isfinite(kth)]
    edge = float(kth.median().item()) if kth.numel() else 0.0
    return edge if 0.0 < edge < float('inf') else 1.0


def knn_search(points, k, lengths=None, grid=None, cell=None):
    """The k nearest neighbours (1 <= k <= 64, open3d KDTreeSearchParamKNN) of every point f32[n,3] (device; several clouds stacked when
    `lengths` int[nc] is given) inside its own cloud, itself included -> (idx int32[n,k], d2 f32[n,k]): ascending by (d2, index),
    padded with n / +inf where the cloud holds fewer than k finite points.  One CellGrid (grid: one built elsewhere over the same points
    and lengths, at any radius; cell: the edge to build one with; neither: a pilot's median k-th distance, the call's one host wait)
    and one buf_grid_knn launch in the grid's order (include/buffer_hip.h N14).  The cell edge affects speed only."""
    if int(k) != k or not 1 <= int(k) <= 64:
        raise ValueError(f"knn_search: k={k} (1 <= k <= 64)")
    if cell is not None and not (0.0 < float(cell) < float('inf')):
        raise ValueError(f"knn_search: cell={cell} (finite, > 0)")
    if cell is not None and grid is not None:
        raise ValueError("knn_search: both a grid and a cell edge given")
    pts, lens = _stacked("knn_search", points, lengths)
    n = int(pts.shape[0])
    if grid is not None and (grid.ns != n or not np.array_equal(grid.s_lengths, lens)):
        raise ValueError("knn_search: the given grid does not cover these clouds")
    if n == 0:
        return (torch.zeros((0, int(k)), dtype=torch.int32, device=pts.device), torch.zeros((0, int(k)), dtype=torch.float32, device=pts.device))
    if grid is None:
        grid = ops.CellGrid(pts, lens, float(cell) if cell is not None else _knn_pilot_cell(pts, lens, k))
    return ops.grid_knn(grid, grid.supports, lens, int(k), q_order=grid.order, return_d2=True)


def nearest_neighbor_distance(points, lengths=None):
    """open3d compute_nearest_neighbor_distance: f64[n], sqrt((double) d2) of column 1 of the k = 2 rows of knn_search -- the distance
    from every point to the nearest OTHER point of its cloud: 0 for a duplicate, +inf for a one-point cloud (and for a non-finite point)."""
    idx, d2 = knn_search(points, 2, lengths)
    return d2[:, 1].double().sqrt()


def cloud_resolution(points, lengths=None):
    """The mean nearest-neighbour distance of every cloud over its finite values (open3d's usual `resolution`) -> f64[nc] on the device;
    NaN for a cloud without a finite value."""
    pts, lens = _stacked("cloud_resolution", points, lengths)
    d = nearest_neighbor_distance(pts, lens)
    seg = torch.repeat_interleave(torch.arange(len(lens), device=d.device), torch.as_tensor(lens, dtype=torch.int64, device=d.device))
    ok = torch.isfinite(d)
    s = torch.zeros(len(lens), dtype=torch.float64, device=d.device).index_add_(0, seg[ok], d[ok])
    c = torch.zeros(len(lens), dtype=torch.float64, device=d.device).index_add_(0, seg[ok], torch.ones_like(d[ok]))
    return s / c


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=2.0, lengths=None):
    """open3d remove_statistical_outlier (0.13, restated: include/buffer_hip.h N15 holds the rule) for stacked clouds ->
    (keep bool[n], new_lengths int32[nc] on the host, mean_i f64[n], [mu, sd, thr] f64[nc,3]).  mean_i = the mean distance from a point
    to its nb_neighbors nearest (itself counted); a point stays iff 0 < mean_i < mu + std_ratio * sd of its cloud.  knn_search, then
    buf_outlier_statistical (fixed summation order: a cloud's numbers are the same bits alone or stacked); one read-back, the counts
    (behind knn_search's pilot)."""
    if int(nb_neighbors) != nb_neighbors or not 1 <= int(nb_neighbors) <= 64:
        raise ValueError(f"remove_statistical_outlier: nb_neighbors={nb_neighbors} (1 <= nb_neighbors <= 64)")
    if not float(std_ratio) > 0.0:
        raise ValueError(f"remove_statistical_outlier: std_ratio={std_ratio} (> 0)")         # open3d: std_ratio <= 0 is an error
    pts, lens = _stacked("remove_statistical_outlier", points, lengths)
    L = _lib.lib()
    n, nc, k = int(pts.shape[0]), int(lens.shape[0]), int(nb_neighbors)
    _, d2 = knn_search(pts, k, lens)
    mean = torch.empty((n,), dtype=torch.float64, device=pts.device)
    stats = torch.empty((nc, 3), dtype=torch.float64, device=pts.device)
    keep = torch.empty((n,), dtype=torch.uint8, device=pts.device)
    kept = torch.empty((nc,), dtype=torch.int32, device=pts.device)
    nbytes = L.buf_outlier_statistical_ws_bytes(nc)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    check(L.buf_outlier_statistical(_ptr(d2), n, k, lens.ctypes.data_as(C.c_void_p), nc, float(std_ratio), _ptr(mean), _ptr(stats),
                                    _ptr(keep), _ptr(kept), _ptr(ws), nbytes, _stream()), "buf_outlier_statistical")
    return keep.bool(), kept.cpu().numpy(), mean, stats


def remove_radius_outlier(points, nb_points, radius, lengths=None):
    """open3d remove_radius_outlier for stacked clouds -> (keep bool[n], new_lengths int32[nc] on the host): a point stays iff more than
    nb_points points of its cloud, itself counted, lie within `radius` of it (d2 < r * r in fp32, the grid's test).  The untruncated
    counts of one count-only CellGrid.query; one read-back, the per-cloud counts."""
    if int(nb_points) != nb_points or int(nb_points) < 0:
        raise ValueError(f"remove_radius_outlier: nb_points={nb_points} (an integer >= 0)")
    r = float(radius)
    if not (0.0 < r < float('inf')):
        raise ValueError(f"remove_radius_outlier: radius={radius} (finite, > 0)")
    pts, lens = _stacked("remove_radius_outlier", points, lengths)
    n = int(pts.shape[0])
    if n == 0:
        return torch.zeros((0,), dtype=torch.bool, device=pts.device), np.zeros(len(lens), np.int32)
    grid = ops.CellGrid(pts, lens, r)
    _, cnt = grid.query(pts, lens, 0, radius=r, q_order=grid.order, counts=True)
    keep = cnt > int(nb_points)
    seg = torch.repeat_interleave(torch.arange(len(lens), device=pts.device), torch.as_tensor(lens, dtype=torch.int64, device=pts.device))
    kept = torch.zeros(len(lens), dtype=torch.int64, device=pts.device).index_add_(0, seg, keep.long())
    return keep, kept.cpu().numpy().astype(np.int32)


def estimate_normals_knn(points, knn=30, camera=(0.0, 0.0, 0.0), orient=True, lengths=None, return_cov=False):
    """open3d estimate_normals(KDTreeSearchParamKNN(knn)) [+ orient_normals_towards_camera_location(camera)] in one pass: knn_search,
    then ops.row_normals on those rows (the arithmetic of estimate_normals_radius on the knn nearest points, the point itself counted)
    -> unit normals f32[n,3] (, covariances f64[n,6]).  Two launches behind the grid build, no retry loop, nothing read back after
    the pilot.  Not bit-equal to estimate_normals, which re-ranks 40 fp32 candidates in fp64 and sums about the origin."""
    if int(knn) != knn or not 1 <= int(knn) <= 64:
        raise ValueError(f"estimate_normals_knn: knn={knn} (1 <= knn <= 64)")
    pts, lens = _stacked("estimate_normals_knn", points, lengths)
    if int(pts.shape[0]) == 0:
        out = torch.zeros((0, 3), dtype=torch.float32, device=pts.device)
        return (out, torch.zeros((0, 6), dtype=torch.float64, device=pts.device)) if return_cov else out
    idx, _ = knn_search(pts, int(knn), lens)
    return ops.row_normals(pts, idx, 0, camera if orient else None, return_cov=return_cov)


def denoise_clouds(points, lengths, denoise):
    """The `denoise` option of prepare_fragments on stacked clouds f32[n,3]: dict(method='statistical', nb_neighbors=20, std_ratio=2.0)
    or dict(method='radius', nb_points=16, radius=...) -> (keep bool[n], new_lengths int32[nc] on the host)."""
    opt = dict(denoise)
    method = opt.pop('method', None)
    if method == 'statistical':
        nb, ratio = opt.pop('nb_neighbors', 20), opt.pop('std_ratio', 2.0)
        if opt:
            raise ValueError(f"denoise: unknown option(s) {sorted(opt)} for method 'statistical'")
        return remove_statistical_outlier(points, nb, ratio, lengths)[:2]
    if method == 'radius':
        if 'radius' not in opt:
            raise ValueError("denoise: method 'radius' needs a radius")
        nb, radius = opt.pop('nb_points', 16), opt.pop('radius')
        if opt:
            raise ValueError(f"denoise: unknown option(s) {sorted(opt)} for method 'radius'")
        return remove_radius_outlier(points, nb, radius, lengths)
    raise ValueError(f"denoise: method={method!r} ('statistical' or 'radius')")


def prepare_fragments(raws, downsample, voxel_size_0, max_num_pts=30000, seeds=None, with_normals=True, denoise=None):
    """The test-split branch of ThreeDMatchDataset.__getitem__ (dataset.py:93-95,125-153) for SEVERAL fragments:
    raws: list of f32[n,3] device tensors -> list of dict(fds_pts f32[N,3] shuffled, sds_pts f32[M,6] = shuffled
    second-level points + normals).  The two voxel levels and the shuffles run per fragment (second level on the first
    level's fp64 means, like open3d's chained calls; fragment i shuffles with the keyed permutation of seeds[i]); the 30-NN normals of
    all fragments are estimated in ONE stacked pass.  Fragment by fragment the result is that of prepare_fragment."""
    seeds = list(range(len(raws))) if seeds is None else list(seeds)
    out, sds_all = [], []
    if not raws:
        return out
    # both voxel levels for all fragments at once (second level on the first level's fp64 means: chained open3d calls)
    fds_all, fds_lens = voxel_down_sample_batch(torch.cat(raws) if len(raws) > 1 else raws[0], [int(r.shape[0]) for r in raws], downsample)
    removed = None
    if denoise is not None:                # outlier removal on the first level (fp32 cast of the means), all fragments in one stacked pass
        keep, kept_lens = denoise_clouds(fds_all.float(), fds_lens, denoise)
        removed = 1.0 - kept_lens / np.maximum(fds_lens, 1)
        fds_all, fds_lens = fds_all[keep], kept_lens.astype(fds_lens.dtype)
    sds_all64, sds_lens = voxel_down_sample_batch(fds_all, fds_lens, voxel_size_0)
    fds32, sds32_all = fds_all.float(), sds_all64.float()
    fo = np.concatenate([[0], np.cumsum(fds_lens)])
    so = np.concatenate([[0], np.cumsum(sds_lens)])
    levels, keys = [], []
    for i, seed in enumerate(seeds):
        levels += [fds32[fo[i]:fo[i + 1]], sds32_all[so[i]:so[i + 1]]]
        # salted: the pipeline permutes the support clouds of pair `seed` with perm_key(seed, 0 / 1) itself
        keys += [ops.perm_key(seed, 0) ^ _SHUFFLE_SALT, ops.perm_key(seed, 1) ^ _SHUFFLE_SALT]
    # np.random.shuffle of both levels (dataset.py:95,112): a keyed pseudo-random permutation per cloud, ONE launch for all of
    # them (torch.randperm is a radix sort per call)
    stacked, lens = ops.permute_clouds(levels, keys)
    offs = np.concatenate([[0], np.cumsum(lens)])
    for i, seed in enumerate(seeds):
        fds32 = stacked[offs[2 * i]:offs[2 * i + 1]]
        sds32 = stacked[offs[2 * i + 1]:offs[2 * i + 2]]
        if sds32.shape[0] > max_num_pts:                                                       # dataset.py:131-137
            g = torch.Generator(device=sds32.device).manual_seed(int(seed))
            sds32 = sds32[torch.randperm(sds32.shape[0], generator=g, device=sds32.device)[:max_num_pts]]
        out.append(dict(fds_pts=fds32.contiguous()))
        sds_all.append(sds32.contiguous())
    if with_normals and sds_all:
        lens = [int(s.shape[0]) for s in sds_all]
        nrm = estimate_normals(torch.cat(sds_all), lengths=lens)
        lo = 0
        for i, s in enumerate(sds_all):
            sds_all[i] = torch.cat([s, nrm[lo:lo + lens[i]]], dim=1).contiguous()
            lo += lens[i]
    for i, (o, s) in enumerate(zip(out, sds_all)):
        o['sds_pts'] = s
        if removed is not None:
            o['denoise_removed'] = float(removed[i])     # fraction of the fragment's first-level points the filter took out
    return out


def prepare_fragment(raw_points, downsample, voxel_size_0, max_num_pts=30000, seed=0, with_normals=True, denoise=None):
    """One fragment of prepare_fragments: raw f32[n,3] -> dict(fds_pts f32[N,3] shuffled, sds_pts f32[M,6])."""
    return prepare_fragments([raw_points], downsample, voxel_size_0, max_num_pts, [seed], with_normals, denoise)[0]
