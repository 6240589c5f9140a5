"""Device operators: torch tensors in HBM -> libbuffer_hip.so kernels on the current HIP stream.

PyTorch is used for device memory and stream handles only; every operator below is a hand-written
gfx950 kernel behind the C ABI of include/buffer_hip.h.  Nothing here falls back to the CPU.
"""
import ctypes as C
import time
import os
import numpy as np
import torch

from . import _lib
from ._lib import buf_grid_t, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.BufferHipError(f"{what}: expected a tensor in device memory (buffer_amd has no CPU path)")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _host_i32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _hptr(a):
    return C.c_void_p(a.ctypes.data)


class CellGrid:
    """Uniform cell grid over stacked support clouds (A2 build half: buf_grid_build)."""

    def __init__(self, supports, s_lengths, radius, cells_per_elem=0):
        L = _lib.lib()
        self.supports = _dev(supports, torch.float32, "CellGrid.supports")
        if self.supports.dim() != 2 or self.supports.shape[1] != 3:
            raise _lib.BufferHipError("Wrong dimensions : support.shape is not (N, 3)")
        self.s_lengths = _host_i32(s_lengths)
        self.ns = int(self.supports.shape[0])
        self.nb = int(self.s_lengths.shape[0])
        self.radius = float(radius)
        if cells_per_elem <= 0:
            cells_per_elem = L.buf_grid_default_cells(self.ns, self.nb)
            f = int(os.environ.get('BUF_GRID_CELLS_PER_POINT', 0))          # development switch: table cells per support point (library default 16)
            if f > 0:
                per = (self.ns + self.nb - 1) // max(self.nb, 1)
                cells_per_elem = min(cells_per_elem, f * per + 65536)
        nbytes = L.buf_grid_ws_bytes(self.ns, self.nb, cells_per_elem)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.supports.device)
        self.g = buf_grid_t()
        check(L.buf_grid_build(C.byref(self.g), _ptr(self.supports), self.ns, _hptr(self.s_lengths), self.nb,
                               self.radius, cells_per_elem, _ptr(self.ws), nbytes, _stream()), "buf_grid_build")

    @property
    def order(self):
        """int32[ns]: global support index in cell order (a spatially coherent processing order)."""
        n = max(self.ns, 1)
        off = self.g.order - self.ws.data_ptr()
        return self.ws[off:off + 4 * n].view(torch.int32)[:self.ns]

    def query(self, queries, q_lengths, k, radius=None, q_order=None, counts=False, max_count=None):
        """-> int32[nq,k] (+ int32[nq] untruncated counts).  Rows ascending by (d2, index), padded
        with ns.  max_count: optional int32[1] device tensor that is atomically max-ed."""
        L = _lib.lib()
        queries = _dev(queries, torch.float32, "CellGrid.query")
        if queries.dim() != 2 or queries.shape[1] != 3:
            raise _lib.BufferHipError("Wrong dimensions : query.shape is not (N, 3)")
        q_lengths = _host_i32(q_lengths)
        if q_lengths.shape[0] != self.nb:
            raise _lib.BufferHipError("Wrong number of batch elements: different for queries and supports ")
        nq = int(queries.shape[0])
        out = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
        cnt = torch.empty((nq,), dtype=torch.int32, device=queries.device) if counts else None
        if q_order is not None:
            q_order = _dev(q_order, torch.int32, "q_order")
        r = self.radius if radius is None else float(radius)
        todo = torch.empty((max(nq, 1),), dtype=torch.int32, device=queries.device) if (k > 0 or q_order is not None) else None
        check(L.buf_grid_query(C.byref(self.g), _ptr(queries), nq, _hptr(q_lengths), _ptr(q_order), r, int(k),
                               _ptr(out), _ptr(cnt), _ptr(max_count), _ptr(todo), _stream()), "buf_grid_query")
        return (out, cnt) if counts else out

    def knn(self, queries, q_lengths, k, q_order=None, return_d2=False):
        """grid_knn on this grid."""
        return grid_knn(self, queries, q_lengths, k, q_order, return_d2)


def grid_knn(grid, queries, q_lengths, k, q_order=None, return_d2=False):
    """buf_grid_knn: the exact k nearest supports (1 <= k <= 64) of every query f32[nq,3] inside its own batch element of `grid` (a
    CellGrid built at any radius: the cell edge affects speed only) -> int32[nq,k] (, f32[nq,k] squared distances).  Rows ascending by
    (d2, index) like CellGrid.query's, padded with ns (+inf) where the element holds fewer than k finite supports.  q_order int32[nq]
    (a permutation, e.g. CellGrid.order for a self query): the processing order, speed only."""
    if not isinstance(grid, CellGrid):
        raise ValueError("grid_knn: grid is not a CellGrid")
    if int(k) != k or not 1 <= int(k) <= 64:
        raise ValueError(f"grid_knn: k={k} (1 <= k <= 64)")
    queries = _dev(queries, torch.float32, "grid_knn.queries")
    if queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError(f"grid_knn: queries {tuple(queries.shape)} is not [N,3]")
    q_lengths = _host_i32(q_lengths)
    nq = int(queries.shape[0])
    if q_lengths.shape[0] != grid.nb or int(q_lengths.sum()) != nq or (q_lengths < 0).any():
        raise ValueError(f"grid_knn: q_lengths {q_lengths.tolist()[:8]} do not split {nq} queries over the grid's {grid.nb} elements")
    if q_order is not None:
        q_order = _dev(q_order, torch.int32, "grid_knn.q_order")
        if tuple(q_order.shape) != (nq,):
            raise ValueError(f"grid_knn: q_order {tuple(q_order.shape)} is not [{nq}]")
    nbr = torch.empty((nq, int(k)), dtype=torch.int32, device=queries.device)
    d2 = torch.empty((nq, int(k)), dtype=torch.float32, device=queries.device) if return_d2 else None
    check(_lib.lib().buf_grid_knn(C.byref(grid.g), _ptr(queries), nq, _hptr(q_lengths), _ptr(q_order), int(k), _ptr(nbr), _ptr(d2), _stream()),
          "buf_grid_knn")
    return (nbr, d2) if return_d2 else nbr


def radius_neighbors(queries, supports, q_lengths, s_lengths, radius, k=None):
    """batch_query semantics on device: int32[nq, max_count] when k is None (two passes: count, fill)."""
    grid = CellGrid(supports, s_lengths, radius)
    if k is None:
        mc = torch.zeros(1, dtype=torch.int32, device=grid.supports.device)
        grid.query(queries, q_lengths, 0, max_count=mc)
        k = int(mc.item())
    return grid.query(queries, q_lengths, k)


def grid_cell_dims(ext, radius, cells_per_elem):
    """The cell rule of buf_grid_build for a box of extent ext[3] -> (edge float, dims (int, int, int)).  Host arithmetic: no device."""
    e = (C.c_double * 3)(*[float(v) for v in ext])
    edge, dim = C.c_double(), (C.c_int * 3)()
    check(_lib.lib().buf_grid_cell_dims(e, float(radius), int(cells_per_elem), C.byref(edge), dim), "buf_grid_cell_dims")
    return edge.value, tuple(dim)


HOST_WAIT_S = [0.0]        # diagnostics: seconds callers spent blocked in calls that end with a host round trip (subsample row counts)


def grid_subsample_batch(points, lengths, dl, max_p=0, max_cells=0, features=None):
    """subsample_batch on device -> (f32[M,3] device tensor, int32[nb] numpy lengths[, f32[M,fd] feature means]).
    Rows per element in ascending voxel-key order."""
    L = _lib.lib()
    points = _dev(points, torch.float32, "grid_subsample_batch.points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.BufferHipError("Wrong dimensions : points.shape is not (N, 3)")
    lengths = _host_i32(lengths)
    n, nb = int(points.shape[0]), int(lengths.shape[0])
    if max_cells <= 0:
        # bucket table of the counting sort: the result does not depend on it (a bucket holds consecutive voxel keys, ranked by key),
        # the memset + two scan passes over it do cost (64 n cells were 180 MB per call at 32 pairs: most of A1's time)
        max_cells = max(1 << 16, int(os.environ.get('BUF_VOX_CELLS_PER_POINT', 4)) * n, 2 * nb)
    fd = 0
    out_f = None
    if features is not None:
        features = _dev(features, torch.float32, "grid_subsample_batch.features")
        fd = int(features.shape[1])
        out_f = torch.empty((max(n, 1), fd), dtype=torch.float32, device=points.device)
    nbytes = L.buf_grid_subsample_ws_bytes(n, nb, max_cells, fd)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=points.device)
    out_b = np.zeros(nb, np.int32)
    m = C.c_int(0)
    t0 = time.perf_counter()
    check(L.buf_grid_subsample_batch(_ptr(points), n, _hptr(lengths), nb, float(dl), int(max_p), _ptr(features), fd,
                                     _ptr(out), _ptr(out_f), _hptr(out_b), C.byref(m), max_cells, _ptr(ws), nbytes,
                                     _stream()), "buf_grid_subsample_batch")
    HOST_WAIT_S[0] += time.perf_counter() - t0          # the call ends with a stream synchronise (rows per element go to the host)
    if features is not None:
        return out[:m.value], out_b, out_f[:m.value]
    return out[:m.value], out_b


# ----------------------------------------------------------------------------- pointnet2 / knn / svd
def furthest_point_sample(xyz, npoint):
    """xyz f32[B,N,3] -> int32[B,npoint]."""
    L = _lib.lib()
    xyz = _dev(xyz, torch.float32, "furthest_point_sample")
    b, n, _ = xyz.shape
    out = torch.empty((b, npoint), dtype=torch.int32, device=xyz.device)
    nbytes = L.buf_fps_ws_bytes(b, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
    check(L.buf_fps(_ptr(xyz), b, n, int(npoint), _ptr(out), _ptr(ws), nbytes, _stream()), "buf_fps")
    return out


def furthest_point_sample_ragged(xyz, lengths, npoint):
    """clouds of different size stacked in xyz f32[sum(n),3] -> int32[b,npoint] (indices local to each cloud);
    all clouds are sampled concurrently, one workgroup each."""
    L = _lib.lib()
    xyz = _dev(xyz, torch.float32, "furthest_point_sample_ragged")
    lengths = _host_i32(lengths)
    b = int(lengths.shape[0])
    out = torch.empty((b, npoint), dtype=torch.int32, device=xyz.device)
    nbytes = L.buf_fps_ws_bytes(1, int(xyz.shape[0]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
    check(L.buf_fps_ragged(_ptr(xyz), _hptr(lengths), b, int(npoint), _ptr(out), _ptr(ws), nbytes, _stream()),
          "buf_fps_ragged")
    return out


def gather_operation(feat, idx):
    """feat f32[B,C,N], idx int32[B,M] -> f32[B,C,M]."""
    L = _lib.lib()
    feat, idx = _dev(feat, torch.float32, "gather_operation"), _dev(idx, torch.int32, "gather_operation")
    b, c, n = feat.shape
    m = idx.shape[1]
    out = torch.empty((b, c, m), dtype=torch.float32, device=feat.device)
    check(L.buf_gather(_ptr(feat), _ptr(idx), b, c, n, m, _ptr(out), _stream()), "buf_gather")
    return out


def grouping_operation(feat, idx):
    """feat f32[B,C,N], idx int32[B,M,S] -> f32[B,C,M,S]."""
    L = _lib.lib()
    feat, idx = _dev(feat, torch.float32, "grouping_operation"), _dev(idx, torch.int32, "grouping_operation")
    b, c, n = feat.shape
    _, m, s = idx.shape
    out = torch.empty((b, c, m, s), dtype=torch.float32, device=feat.device)
    check(L.buf_group(_ptr(feat), _ptr(idx), b, c, n, m, s, _ptr(out), _stream()), "buf_group")
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    """xyz f32[B,N,3], new_xyz f32[B,M,3] -> int32[B,M,nsample]."""
    L = _lib.lib()
    xyz, new_xyz = _dev(xyz, torch.float32, "ball_query"), _dev(new_xyz, torch.float32, "ball_query")
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    out = torch.zeros((b, m, nsample), dtype=torch.int32, device=xyz.device)
    check(L.buf_ball_query(_ptr(xyz), _ptr(new_xyz), b, n, m, float(radius), int(nsample), _ptr(out), _stream()),
          "buf_ball_query")
    return out


def three_nn(unknown, known):
    L = _lib.lib()
    unknown, known = _dev(unknown, torch.float32, "three_nn"), _dev(known, torch.float32, "three_nn")
    b, n, _ = unknown.shape
    m = known.shape[1]
    dist = torch.empty((b, n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=unknown.device)
    check(L.buf_three_nn(_ptr(unknown), _ptr(known), b, n, m, _ptr(dist), _ptr(idx), _stream()), "buf_three_nn")
    return dist, idx


def select_patches(pts, kpts, radius, nsample, out=None):
    """pts f32[N,3] (already permuted), kpts f32[P,3] -> f32[P,nsample,3] (optionally into a contiguous `out` view)."""
    L = _lib.lib()
    pts, kpts = _dev(pts, torch.float32, "select_patches"), _dev(kpts, torch.float32, "select_patches")
    if out is None:
        out = torch.empty((kpts.shape[0], nsample, 3), dtype=torch.float32, device=pts.device)
    elif not out.is_contiguous() or tuple(out.shape) != (kpts.shape[0], nsample, 3):
        raise _lib.BufferHipError("select_patches: out must be a contiguous [P,nsample,3] tensor")
    check(L.buf_select_patches(_ptr(pts), _ptr(kpts), pts.shape[0], kpts.shape[0], float(radius), int(nsample),
                               _ptr(out), _stream()), "buf_select_patches")
    return out


_MASK64 = (1 << 64) - 1


def perm_key(seed, cloud):
    """64-bit key of the keyed permutation of cloud `cloud` (0 = src, 1 = tgt) of the pair registered with `seed`."""
    x = ((int(seed) * 2 + int(cloud)) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def permute_clouds(clouds, keys):
    """clouds: list of f32[n_c,3] device tensors -> (f32[sum n_c,3] stacked and shuffled cloud by cloud, int32[nc] lengths).
    One launch; the permutation of a cloud depends on its key and length only (patch_embedder.py:97-98's randperm)."""
    L = _lib.lib()
    clouds = [_dev(c, torch.float32, "permute_clouds") for c in clouds]
    lens = np.array([c.shape[0] for c in clouds], np.int32)
    out = torch.empty((int(lens.sum()), 3), dtype=torch.float32, device=clouds[0].device)
    nc = len(clouds)
    ptrs = (C.c_void_p * nc)(*[c.data_ptr() for c in clouds])
    ks = (C.c_ulonglong * nc)(*[int(k) & _MASK64 for k in keys])
    check(L.buf_permute_clouds(ptrs, _hptr(lens), ks, nc, _ptr(out), _stream()), "buf_permute_clouds")
    return out, lens


def select_patches_batched(sup, lengths, kpts, m, radius, nsample, out=None):
    """MiniSpinNet.select_patches for every cloud of a step in one launch: sup f32[sum n_c,3] (the permuted support
    clouds stacked), kpts f32[nc*m,3] (m keypoints per cloud) -> f32[nc*m, nsample, 3]."""
    L = _lib.lib()
    sup = _dev(sup, torch.float32, "select_patches_batched.sup")
    kpts = _dev(kpts, torch.float32, "select_patches_batched.kpts")
    lengths = _host_i32(lengths)
    nc = int(lengths.shape[0])
    if kpts.shape[0] != nc * m:
        raise _lib.BufferHipError(f"select_patches_batched: {kpts.shape[0]} keypoints for {nc} clouds x {m}")
    if out is None:
        out = torch.empty((nc * m, nsample, 3), dtype=torch.float32, device=sup.device)
    nbytes = L.buf_select_patches_batched_ws_bytes(int(sup.shape[0]), nc)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=sup.device)
    check(L.buf_select_patches_batched(_ptr(sup), _hptr(lengths), nc, _ptr(kpts), int(m), float(radius), int(nsample), _ptr(out),
                                       _ptr(ws), nbytes, _stream()), "buf_select_patches_batched")
    return out


def compact_greater(x, threshold):
    """ascending int32 indices i with x[i] > threshold (x f32[n] or [n,1]); one host read-back for the count."""
    L = _lib.lib()
    x = _dev(x, torch.float32, "compact_greater").reshape(-1)
    n = int(x.shape[0])
    idx = torch.empty((max(n, 1),), dtype=torch.int32, device=x.device)
    cnt = torch.zeros((1,), dtype=torch.int32, device=x.device)
    nbytes = L.buf_compact_ws_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(L.buf_compact_greater(_ptr(x), 1, n, float(threshold), _ptr(idx), _ptr(cnt), _ptr(ws), nbytes, _stream()),
          "buf_compact_greater")
    return idx[:int(cnt.item())]


def knn(ref, query, k):
    """ref f32[B,N,D], query f32[B,Q,D] -> (dist f32[B,Q,k], idx int64[B,Q,k])."""
    L = _lib.lib()
    ref, query = _dev(ref, torch.float32, "knn"), _dev(query, torch.float32, "knn")
    b, n, d = ref.shape
    q = query.shape[1]
    dist = torch.empty((b, q, k), dtype=torch.float32, device=ref.device)
    idx = torch.empty((b, q, k), dtype=torch.int64, device=ref.device)
    nbytes = L.buf_knn1_ws_bytes(b, n, q) if (int(k) == 1 and d == 32 and n > 0) else L.buf_knn_ws_bytes(b, q, int(k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ref.device)
    check(L.buf_knn(_ptr(ref), _ptr(query), b, n, q, d, int(k), _ptr(dist), _ptr(idx), _ptr(ws), nbytes, _stream()),
          "buf_knn")
    return dist, idx


def svd3x3(a):
    """a f32[B,3,3] -> (U, S, V), a = U diag(S) V^T."""
    L = _lib.lib()
    a = _dev(a, torch.float32, "svd3x3")
    n = a.shape[0]
    u, v = torch.empty_like(a), torch.empty_like(a)
    s = torch.empty((n, 3), dtype=torch.float32, device=a.device)
    check(L.buf_svd3x3_batched(_ptr(a), n, _ptr(u), _ptr(s), _ptr(v), _stream()), "buf_svd3x3_batched")
    return u, s, v


# ----------------------------------------------------------------------------- VN blocks
class VnLayer:
    """Device copy of one VNLinearLeakyReLU (map_to_feat / map_to_dir / VN batch-norm folded)."""

    def __init__(self, W, prefix, device, slope=0.2, linear_only=False):
        if linear_only:
            self.wf = torch.as_tensor(W[prefix + '.weight'], dtype=torch.float32, device=device).contiguous()
            self.wd = self.bsc = self.bsh = None
        else:
            self.wf = torch.as_tensor(W[prefix + '.map_to_feat.weight'], dtype=torch.float32, device=device).contiguous()
            self.wd = torch.as_tensor(W[prefix + '.map_to_dir.weight'], dtype=torch.float32, device=device).contiguous()
            self.bsc = self.bsh = None
            if self.wf.shape[0] != 1:                                  # vn_layers.py:123
                g = np.asarray(W[prefix + '.batchnorm.bn.weight'], np.float64)
                b = np.asarray(W[prefix + '.batchnorm.bn.bias'], np.float64)
                m = np.asarray(W[prefix + '.batchnorm.bn.running_mean'], np.float64)
                v = np.asarray(W[prefix + '.batchnorm.bn.running_var'], np.float64)
                sc = g / np.sqrt(v + 1e-5)
                self.bsc = torch.tensor(sc, dtype=torch.float32, device=device)
                self.bsh = torch.tensor(b - m * sc, dtype=torch.float32, device=device)
        self.cout, self.cin = int(self.wf.shape[0]), int(self.wf.shape[1])
        self.slope = float(slope)


PF_BYTES = [0.0]           # diagnostics (bench.py): bytes of the hoisted form's PF table written + re-read by the calls so far (48 * cout * ns each)


def vn_gather_block(layer, q_pts, s_pts, feats, idx, mode, scale=1.0):
    """VNNBlock / conv half of VNNResnetBlock -> f32[nq, 3*cout]."""
    L = _lib.lib()
    nq, k = idx.shape
    ns = s_pts.shape[0]
    cin = feats.shape[1] // 3
    out = torch.empty((nq, 3 * layer.cout), dtype=torch.float32, device=feats.device)
    if int(mode) == 1 and not os.environ.get('BUF_VN_GATHER_DIRECT') and L.buf_vn_gather_pre_supported(k, cin, layer.cout):
        # the channel contraction once per support point instead of once per neighbour slot (csrc/vn.hip, round 4); a neighbour
        # limit past its LDS stage (k > 96) runs on the direct kernel below, which takes any k
        wsb = L.buf_vn_gather_pre_ws_bytes(ns, layer.cout)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=feats.device)
        PF_BYTES[0] += 48.0 * layer.cout * ns               # PF[j] = [Wf f_j | Wd f_j]: 2 * cout vectors of 12 B per support row, written once and read back
        check(L.buf_vn_gather_block_pre(_ptr(q_pts), _ptr(s_pts), _ptr(feats), _ptr(idx), nq, ns, k, cin, layer.cout, float(scale),
                                        _ptr(layer.wf), _ptr(layer.wd), _ptr(layer.bsc), _ptr(layer.bsh), layer.slope, _ptr(out),
                                        _ptr(ws), wsb, _stream()), "buf_vn_gather_block_pre")
        return out
    check(L.buf_vn_gather_block(_ptr(q_pts), _ptr(s_pts), _ptr(feats), _ptr(idx), nq, ns, k, cin, layer.cout, int(mode),
                                float(scale), _ptr(layer.wf), _ptr(layer.wd), _ptr(layer.bsc), _ptr(layer.bsh),
                                layer.slope, _ptr(out), _stream()), "buf_vn_gather_block")
    return out


def vn_pointwise(layer, b, a=None, ind_a=None, residual=None):
    """VN layer on concat(a[ind_a[:,0]], b) (+ residual) -> f32[n, 3*cout]."""
    L = _lib.lib()
    n = b.shape[0] if b is not None else (ind_a.shape[0] if ind_a is not None else a.shape[0])
    ca = a.shape[1] // 3 if a is not None else 0
    cb = b.shape[1] // 3 if b is not None else 0
    dev = (b if b is not None else a).device
    out = torch.empty((n, 3 * layer.cout), dtype=torch.float32, device=dev)
    stride = ind_a.shape[1] if ind_a is not None else 0
    check(L.buf_vn_pointwise(_ptr(a), _ptr(ind_a), stride, a.shape[0] if a is not None else 0, ca, _ptr(b), cb, n,
                             layer.cout, _ptr(layer.wf), _ptr(layer.wd), _ptr(layer.bsc), _ptr(layer.bsh), layer.slope,
                             _ptr(residual), _ptr(out), _stream()), "buf_vn_pointwise")
    return out


def gather_max(feats, idx):
    L = _lib.lib()
    nq, k = idx.shape
    out = torch.empty((nq, feats.shape[1]), dtype=torch.float32, device=feats.device)
    check(L.buf_gather_max(_ptr(feats), _ptr(idx), nq, feats.shape[0], k, feats.shape[1], _ptr(out), _stream()),
          "buf_gather_max")
    return out


def vn_std(x, z):
    L = _lib.lib()
    n, c = x.shape[0], x.shape[1] // 3
    out = torch.empty((n, 3 * c), dtype=torch.float32, device=x.device)
    check(L.buf_vn_std(_ptr(x), _ptr(z), n, c, _ptr(out), _stream()), "buf_vn_std")
    return out


# ----------------------------------------------------------------------------- patch voxelisation
def patch_voxelize(patches, axis, des_r, centres, azi_cs, voxel_r, nsample, mlp_w, mlp_b, bn_scale, bn_shift,
                   azi_n=20, want_patches=False):
    """patches f32[P,S,3] -> (x f32[P,16,ncentres], R f32[P,3,3], rand_axis f32[P,3], patches_norm|None)."""
    L = _lib.lib()
    P, S, _ = patches.shape
    nc = centres.shape[0]
    dev = patches.device
    x = torch.empty((P, 16, nc), dtype=torch.float32, device=dev)
    R = torch.empty((P, 3, 3), dtype=torch.float32, device=dev)
    ra = torch.empty((P, 3), dtype=torch.float32, device=dev)
    pn = torch.empty((P, S, 3), dtype=torch.float32, device=dev) if want_patches else None
    hw = [np.ascontiguousarray(a, dtype=np.float32) for a in (mlp_w, mlp_b, bn_scale, bn_shift)]
    wsb = L.buf_patch_voxelize_ws_bytes(nc)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(L.buf_patch_voxelize(_ptr(patches), _ptr(axis), P, S, float(des_r), _ptr(centres), nc, int(azi_n),
                               _ptr(azi_cs), float(voxel_r), int(nsample), _hptr(hw[0]), _hptr(hw[1]), _hptr(hw[2]),
                               _hptr(hw[3]), _ptr(x), _ptr(R), _ptr(ra), _ptr(pn), _ptr(ws), wsb, _stream()), "buf_patch_voxelize")
    return x, R, ra, pn


def row_linear(x, w, b, activation=None):
    """Conv1d(kernel 1) of the score heads: x f32[n,cin] @ w[cout,cin].T + b, then None | 'sigmoid' | 'softplus'."""
    L = _lib.lib()
    x = _dev(x, torch.float32, "row_linear")
    n, cin = int(x.shape[0]), int(x.shape[1])
    cout = int(w.shape[0])
    out = torch.empty((n, cout), dtype=torch.float32, device=x.device)
    act = {None: 0, 'sigmoid': 1, 'softplus': 2}[activation]
    check(L.buf_row_linear(_ptr(x), n, cin, cout, _ptr(w.contiguous()), _ptr(b.contiguous()), act, _ptr(out), _stream()),
          "buf_row_linear")
    return out


def score_head(x, seg_lengths, vn1, vn2, lin, w, b, final, eps=1e-5):
    """One score head (VNStdFeature + Conv1d / InstanceNorm1d stack, point_learner.py:128-136,163-171) in 7 launches:
    x f32[n,30], seg_lengths int[nseg] (host: rows per pair), vn1 / vn2 / lin VnLayer, w / b the three Conv1d layers -> f32[n,1]."""
    L = _lib.lib()
    x = _dev(x, torch.float32, "score_head")
    n = int(x.shape[0])
    lens = _host_i32(seg_lengths)
    nseg = int(lens.shape[0])
    out = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    nbytes = L.buf_score_head_ws_bytes(n, nseg)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    act = {None: 0, 'sigmoid': 1, 'softplus': 2}[final]
    check(L.buf_score_head(_ptr(x), n, _hptr(lens), nseg, _ptr(vn1.wf), _ptr(vn1.wd), _ptr(vn1.bsc), _ptr(vn1.bsh), vn1.slope,
                           _ptr(vn2.wf), _ptr(vn2.wd), _ptr(vn2.bsc), _ptr(vn2.bsh), vn2.slope, _ptr(lin.wf),
                           _ptr(w[0]), _ptr(b[0]), _ptr(w[1]), _ptr(b[1]), int(w[1].shape[0]), _ptr(w[2]), _ptr(b[2]), act, float(eps),
                           _ptr(out), _ptr(ws), nbytes, _stream()), "buf_score_head")
    return out


def score_head_supported(x_width, vn1, vn2, lin, w):
    """the fused head exists for the released widths only (10 -> 10 -> 5 -> 3 vector channels, Conv1d 30 -> 20 -> c <= 10 -> 1)"""
    return (x_width == 30 and tuple(vn1.wf.shape) == (10, 10) and tuple(vn2.wf.shape) == (5, 10) and tuple(lin.wf.shape) == (3, 5)
            and vn1.wd is not None and vn2.wd is not None and tuple(w[0].shape) == (20, 30) and w[1].shape[1] == 20 and w[1].shape[0] <= 10
            and tuple(w[2].shape) == (1, int(w[1].shape[0])))


def segment_instance_norm(x, seg_lengths, eps=1e-5):
    """InstanceNorm1d (biased variance) over contiguous row segments: x f32[n,c], seg_lengths int[nseg] (host) -> f32[n,c]."""
    L = _lib.lib()
    x = _dev(x, torch.float32, "segment_instance_norm")
    n, c = int(x.shape[0]), int(x.shape[1])
    lens = _host_i32(seg_lengths)
    nseg = int(lens.shape[0])
    out = torch.empty_like(x)
    nbytes = L.buf_segment_instance_norm_ws_bytes(nseg, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(L.buf_segment_instance_norm(_ptr(x), n, c, _hptr(lens), nseg, float(eps), _ptr(out), _ptr(ws), nbytes, _stream()),
          "buf_segment_instance_norm")
    return out


# ----------------------------------------------------------------------------- pose recovery
def hypotheses_score(ind, ss_kpts, tt_kpts, ss_R, tt_R, azi_n=20, inlier_th=1 / 3):
    L = _lib.lib()
    m = ind.shape[0]
    dev = ind.device
    R = torch.empty((m, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((m, 3), dtype=torch.float32, device=dev)
    num = torch.empty((m,), dtype=torch.int32, device=dev)
    best = torch.zeros((1,), dtype=torch.int32, device=dev)
    mask = torch.zeros((m,), dtype=torch.uint8, device=dev)
    check(L.buf_hypotheses_score(_ptr(ind.contiguous()), _ptr(ss_kpts.contiguous()), _ptr(tt_kpts.contiguous()),
                                 _ptr(ss_R.contiguous()), _ptr(tt_R.contiguous()), m, int(azi_n), float(inlier_th),
                                 _ptr(R), _ptr(t), _ptr(num), _ptr(best), _ptr(mask), _stream()),
          "buf_hypotheses_score")
    return R, t, num, best, mask


def ransac_kabsch(src, tgt, corr, nhyp=4096, seed=0, max_dist=0.10, edge_similarity=0.8):
    """-> (T f32[4,4], info int32[2])."""
    L = _lib.lib()
    dev = src.device
    corr = _dev(corr, torch.int32, "ransac_kabsch")
    T = torch.empty((4, 4), dtype=torch.float32, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    nbytes = L.buf_ransac_ws_bytes(int(nhyp))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_ransac_kabsch(_ptr(src.contiguous()), _ptr(tgt.contiguous()), _ptr(corr), corr.shape[0], int(nhyp),
                              int(seed), float(max_dist), float(edge_similarity), _ptr(T), _ptr(info), _ptr(ws), nbytes,
                              _stream()), "buf_ransac_kabsch")
    return T, info


def ransac_kabsch_masked(src, tgt, mask, nhyp=4096, seed=0, max_dist=0.10, edge_similarity=0.8):
    """ransac_kabsch on the correspondences with mask != 0 (uint8[m]); nothing returns to the host.
    -> (T f32[4,4], info int32[2])."""
    L = _lib.lib()
    dev = src.device
    mask = _dev(mask, torch.uint8, "ransac_kabsch_masked")
    m = int(mask.shape[0])
    T = torch.empty((4, 4), dtype=torch.float32, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    nbytes = L.buf_ransac_masked_ws_bytes(m, int(nhyp))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_ransac_kabsch_masked(_ptr(src.contiguous()), _ptr(tgt.contiguous()), _ptr(mask), m, int(nhyp), int(seed),
                                     float(max_dist), float(edge_similarity), _ptr(T), _ptr(info), _ptr(ws), nbytes, _stream()),
          "buf_ransac_kabsch_masked")
    return T, info


def post_refine(T_init, src, tgt, thr=0.10, iters=20):
    L = _lib.lib()
    dev = src.device
    T_init = _dev(T_init, torch.float32, "post_refine").reshape(4, 4)
    T = torch.empty((4, 4), dtype=torch.float32, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    check(L.buf_post_refine(_ptr(T_init), _ptr(src.contiguous()), _ptr(tgt.contiguous()), src.shape[0], float(thr),
                            int(iters), _ptr(T), _ptr(info), _stream()), "buf_post_refine")
    return T, info


def _icp_outputs(B, dev):
    """The (T f64[B,4,4], fitness f64[B], rmse f64[B], iterations int32[B]) outputs of icp_batched / vgicp_batched."""
    return (torch.empty((B, 4, 4), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.float64, device=dev),
            torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))


ICP_METHODS = {'point_to_point': 0, 'point_to_plane': 1, 'generalized': 2}     # BUF_ICP_POINT_TO_POINT / _POINT_TO_PLANE / _GENERALIZED


def icp_batched(src, src_lengths, tgt, tgt_lengths, max_dist, T_init, method='point_to_point', tgt_normals=None, max_iteration=30,
                relative_fitness=1e-6, relative_rmse=1e-6, correspondences=False, src_normals=None, epsilon=1e-3):
    """buf_icp_batched: ICP of the pairs stacked in src f32[sum src_lengths,3] / tgt f32[sum tgt_lengths,3] (pair b owns
    src_lengths[b] / tgt_lengths[b] consecutive rows), T_init f64[B,4,4] -> (T f64[B,4,4], fitness f64[B], rmse f64[B],
    iterations int32[B], nn int32[sum src_lengths] or None: global target row per source point, sum tgt_lengths = no match).
    method 'generalized' goes to buf_gicp_batched with src_normals (shaped like src), tgt_normals and epsilon."""
    L = _lib.lib()
    src, tgt = _dev(src, torch.float32, "icp_batched.src"), _dev(tgt, torch.float32, "icp_batched.tgt")
    sl, tl = _host_i32(src_lengths), _host_i32(tgt_lengths)
    B, dev = int(sl.shape[0]), src.device
    m = ICP_METHODS[method]
    nrm = _dev(tgt_normals, torch.float32, "icp_batched.tgt_normals") if tgt_normals is not None else None
    T_init = _dev(T_init, torch.float64, "icp_batched.T_init").reshape(B, 4, 4)
    T, fit, rmse, iters = _icp_outputs(B, dev)
    nn = torch.empty((max(int(src.shape[0]), 1),), dtype=torch.int32, device=dev) if correspondences else None
    nbytes = max(L.buf_icp_ws_bytes(int(src.shape[0]), int(tgt.shape[0]), max(B, 1), m), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if method == 'generalized':
        if src_normals is None or nrm is None:
            raise ValueError("icp_batched: method 'generalized' needs src_normals and tgt_normals")
        if not (0.0 < float(epsilon) <= 1.0):
            raise ValueError(f"icp_batched: epsilon={epsilon} (must be in (0, 1])")
        snrm = _dev(src_normals, torch.float32, "icp_batched.src_normals")
        if tuple(snrm.shape) != tuple(src.shape) or tuple(nrm.shape) != tuple(tgt.shape):
            raise ValueError("icp_batched: src_normals / tgt_normals must be shaped like src / tgt")
        check(L.buf_gicp_batched(_ptr(src), _ptr(snrm), _hptr(sl), _ptr(tgt), _ptr(nrm), _hptr(tl), B, float(max_dist), float(epsilon),
                                 _ptr(T_init), int(max_iteration), float(relative_fitness), float(relative_rmse), _ptr(T), _ptr(fit),
                                 _ptr(rmse), _ptr(iters), _ptr(nn), _ptr(ws), nbytes, _stream()), "buf_gicp_batched")
    else:
        check(L.buf_icp_batched(_ptr(src), _hptr(sl), _ptr(tgt), _ptr(nrm), _hptr(tl), B, m, float(max_dist), _ptr(T_init),
                                int(max_iteration), float(relative_fitness), float(relative_rmse), _ptr(T), _ptr(fit), _ptr(rmse),
                                _ptr(iters), _ptr(nn), _ptr(ws), nbytes, _stream()), "buf_icp_batched")
    return T, fit, rmse, iters, (nn[:int(src.shape[0])] if nn is not None else None)


VGICP_NEIGHBORS = (1, 7, 27)
VOXEL_MAP_CELLS = (1 << 22, 1 << 25, 1 << 28)     # table sizes voxel_map_build tries in turn when max_cells is not given


class VoxelMap:
    """A built voxel map (include/buffer_hip.h, N9): the device buffer `buf` that holds it, the host handle `m` into it, nclouds, voxel,
    epsilon, nrows (rows of all clouds).  It serves any number of vgicp_batched calls."""

    def __init__(self, m, buf):
        self.m, self.buf = m, buf
        self.nclouds, self.nrows, self.voxel, self.epsilon = int(m.nclouds), int(m.nrows), float(m.voxel), float(m.epsilon)

    def rows(self):
        """buf_voxel_map_export -> dict of device tensors: keys int64[R], counts int32[R], means f64[R,3], covs f64[R,6] (00 01 02 11 12
        22), row_off int32[nclouds + 1]; rows of a cloud in ascending key order, clouds one after the other."""
        dev, R = self.buf.device, self.nrows
        out = dict(keys=torch.empty((R,), dtype=torch.int64, device=dev), counts=torch.empty((R,), dtype=torch.int32, device=dev),
                   means=torch.empty((R, 3), dtype=torch.float64, device=dev), covs=torch.empty((R, 6), dtype=torch.float64, device=dev),
                   row_off=torch.empty((self.nclouds + 1,), dtype=torch.int32, device=dev))
        check(_lib.lib().buf_voxel_map_export(C.byref(self.m), R, _ptr(out['keys']), _ptr(out['counts']), _ptr(out['means']),
                                              _ptr(out['covs']), _ptr(out['row_off']), _stream()), "buf_voxel_map_export")
        return out


def voxel_map_build(points, lengths, voxel, normals=None, epsilon=1e-3, max_cells=0):
    """buf_voxel_map_build: the voxel map of the clouds stacked in points f32[sum lengths,3] (normals f32 like points, or None: C = I)
    -> VoxelMap.  max_cells bounds the dense lookup table over the clouds' voxel boxes (BufferHipError, BUF_ECAPACITY, when they need
    more); 0: VOXEL_MAP_CELLS are tried in turn.  One small readback per attempt."""
    L = _lib.lib()
    points = _dev(points, torch.float32, "voxel_map_build.points").reshape(-1, 3)
    lengths = _host_i32(lengths)
    n, nb = int(points.shape[0]), int(lengths.shape[0])
    if normals is not None:
        normals = _dev(normals, torch.float32, "voxel_map_build.normals").reshape(-1, 3)
        if tuple(normals.shape) != tuple(points.shape):
            raise ValueError("voxel_map_build: normals must be shaped like points")
    sizes = (int(max_cells),) if max_cells > 0 else VOXEL_MAP_CELLS
    for k, cells in enumerate(sizes):
        nbytes, wbytes = max(L.buf_voxel_map_bytes(n, nb, cells), 1), max(L.buf_voxel_map_ws_bytes(n, nb, cells), 1)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
        ws = torch.empty(wbytes, dtype=torch.uint8, device=points.device)
        m = _lib.buf_voxel_map_t()
        rc = L.buf_voxel_map_build(C.byref(m), _ptr(points), _ptr(normals), _hptr(lengths), nb, float(voxel), float(epsilon), cells,
                                   _ptr(buf), nbytes, _ptr(ws), wbytes, _stream())
        if rc == -4 and k + 1 < len(sizes):                 # BUF_ECAPACITY: the next table size
            continue
        check(rc, "buf_voxel_map_build")
        return VoxelMap(m, buf)


def vgicp_batched(src, src_lengths, vmap, T_init, neighbors=7, src_normals=None, pair_cloud=None, max_iteration=30, rel_fitness=1e-6,
                  rel_rmse=1e-6, rows=False):
    """buf_vgicp_batched: voxelized Generalized ICP of the sources stacked in src f32[sum src_lengths,3] against the clouds of vmap (a
    VoxelMap; pair b uses cloud pair_cloud[b], or cloud b without pair_cloud), T_init f64[B,4,4] -> (T f64[B,4,4], fitness f64[B],
    rmse f64[B], iterations int32[B], row int32[sum src_lengths] or None: the cloud-local map row of the voxel each source point fell
    into in the last pass, -1 = none)."""
    L = _lib.lib()
    if neighbors not in VGICP_NEIGHBORS:
        raise ValueError(f"vgicp_batched: neighbors={neighbors} (one of {VGICP_NEIGHBORS})")
    src = _dev(src, torch.float32, "vgicp_batched.src").reshape(-1, 3)
    sl = _host_i32(src_lengths)
    B, dev, ns = int(sl.shape[0]), src.device, int(src.shape[0])
    snrm = None
    if src_normals is not None:
        snrm = _dev(src_normals, torch.float32, "vgicp_batched.src_normals").reshape(-1, 3)
        if tuple(snrm.shape) != tuple(src.shape):
            raise ValueError("vgicp_batched: src_normals must be shaped like src")
    pc = None
    if pair_cloud is not None:
        pc = _host_i32(pair_cloud)
        if pc.shape[0] != B:
            raise ValueError(f"vgicp_batched: {B} pairs but {pc.shape[0]} pair_cloud entries")
    T_init = _dev(T_init, torch.float64, "vgicp_batched.T_init").reshape(B, 4, 4)
    T, fit, rmse, iters = _icp_outputs(B, dev)
    row = torch.empty((max(ns, 1),), dtype=torch.int32, device=dev) if rows else None
    nbytes = max(L.buf_vgicp_ws_bytes(ns, max(B, 1)), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_vgicp_batched(C.byref(vmap.m), _ptr(src), _ptr(snrm), _hptr(sl), _hptr(pc) if pc is not None else C.c_void_p(0), B,
                              int(neighbors), _ptr(T_init), int(max_iteration), float(rel_fitness), float(rel_rmse), _ptr(T), _ptr(fit),
                              _ptr(rmse), _ptr(iters), _ptr(row), _ptr(ws), nbytes, _stream()), "buf_vgicp_batched")
    return T, fit, rmse, iters, (row[:ns] if row is not None else None)


def fpfh(points, normals, nbr, max_nn=100, return_spfh=False):
    """buf_fpfh: FPFH descriptors of the points f32[n,3] with normals f32[n,3] from their sorted radius rows nbr int32[n,k]
    (CellGrid.query: padded with values >= n; column 0 is the point itself) -> f64[n,33] (, the SPFH table f64[n,33]).  The rows may
    belong to several stacked clouds: a row stays inside its cloud."""
    L = _lib.lib()
    points, normals = _dev(points, torch.float32, "fpfh.points"), _dev(normals, torch.float32, "fpfh.normals")
    nbr = _dev(nbr, torch.int32, "fpfh.nbr")
    if points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError(f"fpfh: points {tuple(points.shape)} and normals {tuple(normals.shape)} are not both [N,3]")
    n = int(points.shape[0])
    if nbr.dim() != 2 or nbr.shape[0] != n:
        raise ValueError(f"fpfh: nbr {tuple(nbr.shape)} is not [{n},k]")
    out = torch.empty((n, 33), dtype=torch.float64, device=points.device)
    spfh = torch.empty((n, 33), dtype=torch.float64, device=points.device)
    check(L.buf_fpfh(_ptr(points), _ptr(normals), n, _ptr(nbr), int(nbr.shape[1]), int(max_nn), _ptr(out), _ptr(spfh), None, 0,
                     _stream()), "buf_fpfh")
    return (out, spfh) if return_spfh else out


def iss_keypoints(points, nbr_sal, nbr_nms, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, max_nn=0, return_eig=True):
    """buf_iss_keypoints: ISS keypoints of the points f32[n,3] from their sorted radius rows at the salient radius nbr_sal int32[n,k]
    and at the non-max radius nbr_nms int32[n,k'] (CellGrid.query: padded with values >= n; the same tensor may serve both) ->
    (mask u8[n], saliency f64[n], eig f64[n,3] descending or None).  max_nn: 0 = whole rows, else the first max_nn columns.  The rows may
    belong to several stacked clouds: a row stays inside its cloud."""
    L = _lib.lib()
    points = _dev(points, torch.float32, "iss_keypoints.points")
    nbr_sal, nbr_nms = _dev(nbr_sal, torch.int32, "iss_keypoints.nbr_sal"), _dev(nbr_nms, torch.int32, "iss_keypoints.nbr_nms")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"iss_keypoints: points {tuple(points.shape)} is not [N,3]")
    n = int(points.shape[0])
    for what, nbr in (("nbr_sal", nbr_sal), ("nbr_nms", nbr_nms)):
        if nbr.dim() != 2 or nbr.shape[0] != n:
            raise ValueError(f"iss_keypoints: {what} {tuple(nbr.shape)} is not [{n},k]")
    mask = torch.empty((n,), dtype=torch.uint8, device=points.device)
    sal = torch.empty((n,), dtype=torch.float64, device=points.device)
    eig = torch.empty((n, 3), dtype=torch.float64, device=points.device) if return_eig else None
    check(L.buf_iss_keypoints(_ptr(points), n, _ptr(nbr_sal), int(nbr_sal.shape[1]), _ptr(nbr_nms), int(nbr_nms.shape[1]), int(max_nn),
                              float(gamma_21), float(gamma_32), int(min_neighbors), _ptr(sal), _ptr(eig), _ptr(mask), _stream()),
          "buf_iss_keypoints")
    return mask, sal, eig


def row_normals(points, nbr, max_nn=0, camera=None, order=None, return_cov=False, return_counts=False):
    """buf_row_normals: normals of the points f32[n,3] from their sorted radius rows nbr int32[n,k] (CellGrid.query: padded with values
    >= n; the point itself is in its row and counts) -> unit normals f32[n,3] (, covariances f64[n,6] = (c00, c01, c02, c11, c12, c22))
    (, row lengths int32[n]).  max_nn: 0 = whole rows, else the first max_nn columns.  camera (3 numbers): the normals are flipped
    towards it; None leaves them as computed.  order int32[n] (a permutation, e.g. CellGrid.order): the processing order, speed only.
    Rows of fewer than 3 points give (0, 0, 1) and the identity.  The rows may belong to several stacked clouds."""
    L = _lib.lib()
    points, nbr = _dev(points, torch.float32, "row_normals.points"), _dev(nbr, torch.int32, "row_normals.nbr")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"row_normals: points {tuple(points.shape)} is not [N,3]")
    n = int(points.shape[0])
    if nbr.dim() != 2 or nbr.shape[0] != n or nbr.shape[1] < 1:
        raise ValueError(f"row_normals: nbr {tuple(nbr.shape)} is not [{n},k], k >= 1")
    if int(max_nn) < 0:
        raise ValueError(f"row_normals: max_nn={max_nn} (0 = whole rows, or >= 1)")
    if order is not None:
        order = _dev(order, torch.int32, "row_normals.order")
        if tuple(order.shape) != (n,):
            raise ValueError(f"row_normals: order {tuple(order.shape)} is not [{n}]")
    cam = None
    if camera is not None:
        cam = np.asarray(camera, np.float64).reshape(-1)
        if cam.shape[0] != 3:
            raise ValueError(f"row_normals: camera holds {cam.shape[0]} numbers, not 3")
        cam = (C.c_double * 3)(*cam.tolist())
    normals = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    cov = torch.empty((n, 6), dtype=torch.float64, device=points.device) if return_cov else None
    cnt = torch.empty((n,), dtype=torch.int32, device=points.device) if return_counts else None
    check(L.buf_row_normals(_ptr(points), n, _ptr(nbr), int(nbr.shape[1]), int(max_nn), _ptr(order), cam, 0 if cam is None else 1,
                            _ptr(normals), _ptr(cov), _ptr(cnt), _stream()), "buf_row_normals")
    out = (normals,) + ((cov,) if return_cov else ()) + ((cnt,) if return_counts else ())
    return out if len(out) > 1 else normals


def _corr_batch(fn, src, src_lengths, tgt, tgt_lengths, corr, corr_lengths):
    """The (src, tgt, corr) batch of fgr_batched / sc2_batched / clique_batched (fn) on the device and its host lengths, checked against
    each other -> (src, tgt, corr, sl, tl, cl, B, dev)."""
    src, tgt = _dev(src, torch.float32, f"{fn}.src"), _dev(tgt, torch.float32, f"{fn}.tgt")
    corr = _dev(corr, torch.int32, f"{fn}.corr")
    sl, tl, cl = _host_i32(src_lengths), _host_i32(tgt_lengths), _host_i32(corr_lengths)
    B = int(sl.shape[0])
    if tl.shape[0] != B or cl.shape[0] != B:
        raise ValueError(f"{fn}: {B} source lengths but {tl.shape[0]} target and {cl.shape[0]} correspondence lengths")
    for name, t, ln, w in (("src", src, sl, 3), ("tgt", tgt, tl, 3), ("corr", corr, cl, 2)):
        if t.dim() != 2 or t.shape[1] != w:
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} is not [N,{w}]")
        if (ln < 0).any() or int(ln.astype(np.int64).sum()) != int(t.shape[0]):
            raise ValueError(f"{fn}: {name} lengths sum to {int(ln.astype(np.int64).sum())}, {name} holds {int(t.shape[0])} rows")
    return src, tgt, corr, sl, tl, cl, B, src.device


def feature_match(fa, a_lengths, fb, b_lengths, mutual=True, ratio=None, return_nn=False):
    """buf_feature_match (N12 of buffer_hip.h): the descriptor matches of the pairs stacked in fa f32|f64[sum a_lengths,d] /
    fb [sum b_lengths,d] (device, 1 <= d <= 64; float64 is cast to fp32, as fpfh.match casts), pair p owning a_lengths[p] / b_lengths[p]
    consecutive rows -> (corr int32[m,2] (device: (row of A_p, its nearest row of B_p), pair-local, ascending inside a pair, the pairs
    stacked: what _corr_batch takes), corr_lengths int32[P] (host), nn, ssd).  mutual: only the rows that are each other's nearest.
    ratio (None = off, else in (0, 1)): only the rows whose nearest squared distance is at most ratio^2 times the second nearest (Lowe's
    test, forward direction).  return_nn: nn int32[sum a_lengths,2] / ssd f32[sum a_lengths,2] = every row's nearest and second-nearest
    row (-1) and squared distance (+inf), else None.  Exact and deterministic; one read-back, the counts."""
    L = _lib.lib()
    fa, fb = _dev(fa, torch.float32, "feature_match.fa"), _dev(fb, torch.float32, "feature_match.fb")
    al, bl = _host_i32(a_lengths), _host_i32(b_lengths)
    P = int(al.shape[0])
    if bl.shape[0] != P:
        raise ValueError(f"feature_match: {P} lengths of A but {bl.shape[0]} of B")
    if fa.dim() != 2 or fb.dim() != 2 or fa.shape[1] != fb.shape[1]:
        raise ValueError(f"feature_match: fa {tuple(fa.shape)} and fb {tuple(fb.shape)} are not [N,d] with one d")
    for name, t, ln in (("fa", fa, al), ("fb", fb, bl)):
        if (ln < 0).any() or int(ln.astype(np.int64).sum()) != int(t.shape[0]):
            raise ValueError(f"feature_match: {name} lengths sum to {int(ln.astype(np.int64).sum())}, {name} holds {int(t.shape[0])} rows")
    if ratio is not None and not (0.0 < float(ratio) < 1.0):
        raise ValueError(f"feature_match: ratio={ratio} (None, or in (0, 1))")
    na, nb, d, dev = int(fa.shape[0]), int(fb.shape[0]), int(fa.shape[1]), fa.device
    corr = torch.empty((na, 2), dtype=torch.int32, device=dev)
    counts = torch.zeros((P,), dtype=torch.int32, device=dev)
    nn = torch.empty((na, 2), dtype=torch.int32, device=dev) if return_nn else None
    ssd = torch.empty((na, 2), dtype=torch.float32, device=dev) if return_nn else None
    nbytes = max(L.buf_feature_match_ws_bytes(na, nb, P), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_feature_match(_ptr(fa), _hptr(al), _ptr(fb), _hptr(bl), P, d, int(bool(mutual)), 0.0 if ratio is None else float(ratio),
                              _ptr(corr), _ptr(counts), _ptr(nn), _ptr(ssd), _ptr(ws), nbytes, _stream()), "buf_feature_match")
    cl = counts.cpu().numpy()
    return corr[:int(cl.sum())], cl, nn, ssd


FGR_STATUS = ('NOTHING', 'OK', 'FAILED')                                                      # BUF_FGR_* of buffer_hip.h
FGR_MAX_TUPLES = 4096


def fgr_batched(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, seeds=None, tuple_scale=0.95, max_tuples=1000, trial_factor=100,
                mu_start=1.0, delta=0.025, delta_absolute=False, division_factor=1.4, decrease_every=4, iterations=64,
                return_rows=False):
    """buf_fgr_batched: Fast Global Registration of the pairs stacked in src f32[sum src_lengths,3] / tgt f32[sum tgt_lengths,3] on
    the correspondences corr int32[sum corr_lengths,2] ((src row, tgt row) inside the pair's own clouds), pair b drawing its tuples
    with seeds[b] (default b) -> (T f64[B,4,4] src -> tgt, info int32[B,4] = (index into FGR_STATUS, tuples kept, trials examined,
    updates applied), rows int32[B,3*max_tuples,2] or None: the kept correspondences, tail -1, weights f64[B,3*max_tuples] or None:
    their line-process weights at the last linearisation, tail NaN), all on the device; two launches, nothing read back."""
    L = _lib.lib()
    src, tgt, corr, sl, tl, cl, B, dev = _corr_batch("fgr_batched", src, src_lengths, tgt, tgt_lengths, corr, corr_lengths)
    if not (1 <= int(max_tuples) <= FGR_MAX_TUPLES):
        raise ValueError(f"fgr_batched: max_tuples={max_tuples} (1..{FGR_MAX_TUPLES})")
    sd = np.arange(B, dtype=np.uint64) if seeds is None else np.array([int(s) & _MASK64 for s in seeds], dtype=np.uint64).reshape(-1)
    if sd.shape[0] != B:
        raise ValueError(f"fgr_batched: {B} pairs but {sd.shape[0]} seeds")
    mt = int(max_tuples)
    T = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
    info = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    rows = torch.empty((B, 3 * mt, 2), dtype=torch.int32, device=dev) if return_rows else None
    weights = torch.empty((B, 3 * mt), dtype=torch.float64, device=dev) if return_rows else None
    nbytes = max(L.buf_fgr_ws_bytes(int(corr.shape[0]), max(B, 1), mt), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_fgr_batched(_ptr(src), _hptr(sl), _ptr(tgt), _hptr(tl), _ptr(corr), _hptr(cl), B, _hptr(sd), float(tuple_scale), mt,
                            int(trial_factor), float(mu_start), float(delta), int(bool(delta_absolute)), float(division_factor),
                            int(decrease_every), int(iterations), _ptr(T), _ptr(info), _ptr(rows), _ptr(weights), _ptr(ws), nbytes,
                            _stream()), "buf_fgr_batched")
    return T, info, rows, weights


SC2_STATUS = ('NOTHING', 'OK')                                                                  # BUF_SC2_* of buffer_hip.h
SC2_MAX_ROWS, SC2_MAX_SEEDS, SC2_MAX_K1 = 16384, 1024, 128


def sc2_batched(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, d_thr, inlier_thr, seed_ratio=0.2, max_seeds=512, k1=30,
                nms_radius=0.0, power_iterations=10, refine_iterations=20, return_detail=False):
    """buf_sc2_batched: SC2-PCR (second order spatial compatibility, single stage) of the pairs stacked in src f32[sum src_lengths,3] /
    tgt f32[sum tgt_lengths,3] on the correspondences corr int32[sum corr_lengths,2] ((src row, tgt row) inside the pair's own
    clouds); deterministic, no seeds -> (T f64[B,4,4] src -> tgt, info int32[B,6] = (index into SC2_STATUS, live rows, seeds, the
    winner's row, its inlier count before refinement, the final count), detail), all on the device, nothing read back.  detail is None
    or, with return_detail=True, dict(confidence f64[sum n] (NaN on dead rows), seeds int32[B,max_seeds] and hyp_counts
    int32[B,max_seeds] (by rank, tail -1), counts int32[max_seeds * sum n] (pair b's block at max_seeds * its first row, rank r at
    + r n_b), inlier_mask uint8[sum n])."""
    L = _lib.lib()
    src, tgt, corr, sl, tl, cl, B, dev = _corr_batch("sc2_batched", src, src_lengths, tgt, tgt_lengths, corr, corr_lengths)
    if B and int(cl.max()) > SC2_MAX_ROWS:
        raise ValueError(f"sc2_batched: {int(cl.max())} correspondences in one pair (at most {SC2_MAX_ROWS})")
    if not (1 <= int(max_seeds) <= SC2_MAX_SEEDS) or not (3 <= int(k1) <= SC2_MAX_K1):
        raise ValueError(f"sc2_batched: max_seeds={max_seeds} (1..{SC2_MAX_SEEDS}), k1={k1} (3..{SC2_MAX_K1})")
    ms, n = int(max_seeds), int(corr.shape[0])
    T = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
    info = torch.zeros((B, 6), dtype=torch.int32, device=dev)
    detail = None
    if return_detail:
        detail = dict(confidence=torch.empty(n, dtype=torch.float64, device=dev), seeds=torch.empty((B, ms), dtype=torch.int32, device=dev),
                      hyp_counts=torch.empty((B, ms), dtype=torch.int32, device=dev),
                      counts=torch.empty(ms * n, dtype=torch.int32, device=dev), inlier_mask=torch.empty(n, dtype=torch.uint8, device=dev))
    d = detail or {}
    nbytes = max(L.buf_sc2_ws_bytes(_hptr(cl), B, ms), 1) if B else 1
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_sc2_batched(_ptr(src), _hptr(sl), _ptr(tgt), _hptr(tl), _ptr(corr), _hptr(cl), B, float(d_thr), float(inlier_thr),
                            float(seed_ratio), ms, int(k1), float(nms_radius), int(power_iterations), int(refine_iterations), _ptr(T),
                            _ptr(info), _ptr(d.get('confidence')), _ptr(d.get('seeds')), _ptr(d.get('hyp_counts')), _ptr(d.get('counts')),
                            _ptr(d.get('inlier_mask')), _ptr(ws), nbytes, _stream()), "buf_sc2_batched")
    return T, info, detail


CLIQUE_STATUS = ('NOTHING', 'OK')                                                               # BUF_CLIQUE_* of buffer_hip.h
CLIQUE_MAX_SEEDS, CLIQUE_MAX_MEMBERS = 1024, 512


def clique_batched(src, src_lengths, tgt, tgt_lengths, corr, corr_lengths, d_thr, tim_thr=None, t_thr=None, inlier_thr=None,
                   max_seeds=64, max_members=256, gnc_factor=1.4, gnc_iterations=100, refine_iterations=20, return_detail=False):
    """buf_clique_batched: greedy maximum clique of the compatibility graph with its k-core bound, GNC-TLS rotation, voted translation
    and SC2's refit (the TEASER-style estimator, N10 of buffer_hip.h) of the pairs stacked in src f32[sum src_lengths,3] / tgt
    f32[sum tgt_lengths,3] on the correspondences corr int32[sum corr_lengths,2] ((src row, tgt row) inside the pair's own clouds);
    deterministic, no seeds; tim_thr and inlier_thr default to d_thr, t_thr to d_thr / 2 -> (T f64[B,4,4] src -> tgt, info int32[B,8] =
    (index into CLIQUE_STATUS, live rows, bound, the winner's size, its rank, members used, GNC steps, the final inlier count),
    detail), all on the device, nothing read back.  detail is None or, with return_detail=True, dict(deg / core / rank int32[sum n]
    (-1 on dead rows), sizes int32[B,max_seeds] (by rank, tail -1), members int32[B,max_members] (rows, tail -1), weights
    f64[B, max_members (max_members - 1) / 2] (NaN tail), pose0 f64[B,12] (R and t before the refit), inlier_mask uint8[sum n])."""
    L = _lib.lib()
    src, tgt, corr, sl, tl, cl, B, dev = _corr_batch("clique_batched", src, src_lengths, tgt, tgt_lengths, corr, corr_lengths)
    if B and int(cl.max()) > SC2_MAX_ROWS:
        raise ValueError(f"clique_batched: {int(cl.max())} correspondences in one pair (at most {SC2_MAX_ROWS})")
    if not (1 <= int(max_seeds) <= CLIQUE_MAX_SEEDS) or not (3 <= int(max_members) <= CLIQUE_MAX_MEMBERS):
        raise ValueError(f"clique_batched: max_seeds={max_seeds} (1..{CLIQUE_MAX_SEEDS}), max_members={max_members} "
                         f"(3..{CLIQUE_MAX_MEMBERS})")
    d_thr = float(d_thr)
    tim_thr = d_thr if tim_thr is None else float(tim_thr)
    t_thr = d_thr / 2 if t_thr is None else float(t_thr)
    inlier_thr = d_thr if inlier_thr is None else float(inlier_thr)
    ms, mm, n = int(max_seeds), int(max_members), int(corr.shape[0])
    T = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
    info = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    detail = None
    if return_detail:
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        detail = dict(deg=i32(n), core=i32(n), rank=i32(n), sizes=i32(B, ms), members=i32(B, mm),
                      weights=torch.empty((B, mm * (mm - 1) // 2), dtype=torch.float64, device=dev),
                      pose0=torch.empty((B, 12), dtype=torch.float64, device=dev), inlier_mask=torch.empty(n, dtype=torch.uint8, device=dev))
    d = detail or {}
    nbytes = max(L.buf_clique_ws_bytes(_hptr(cl), B, ms, mm), 1) if B else 1
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_clique_batched(_ptr(src), _hptr(sl), _ptr(tgt), _hptr(tl), _ptr(corr), _hptr(cl), B, d_thr, tim_thr, t_thr, inlier_thr, ms,
                               mm, float(gnc_factor), int(gnc_iterations), int(refine_iterations), _ptr(T), _ptr(info), _ptr(d.get('deg')),
                               _ptr(d.get('core')), _ptr(d.get('rank')), _ptr(d.get('sizes')), _ptr(d.get('members')),
                               _ptr(d.get('weights')), _ptr(d.get('pose0')), _ptr(d.get('inlier_mask')), _ptr(ws), nbytes, _stream()),
          "buf_clique_batched")
    return T, info, detail


def pair_stats(points, lengths, pair_src, pair_tgt, T, radius, correspondences=False, cells_per_elem=0):
    """buf_pair_stats: statistics of P pairs over the C clouds stacked in points f32[sum lengths,3] under given transforms, one cell
    grid per call, nothing read back.  pair_src / pair_tgt host int[P] (cloud indices), T f64[P,4,4] (device) mapping the source
    cloud into the target cloud's frame -> (matched int32[P], moments f64[P,10] = sum d2, sum u (3), upper triangle of sum u u^T
    (6) over the matched target points u, nn int32[sum of the pairs' source rows] or None: row inside the target cloud, -1 = none)."""
    L = _lib.lib()
    points = _dev(points, torch.float32, "pair_stats.points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"pair_stats: points {tuple(points.shape)} is not [N,3]")
    ln, pa, pb = _host_i32(lengths), _host_i32(pair_src), _host_i32(pair_tgt)
    if pa.shape != pb.shape:
        raise ValueError(f"pair_stats: {pa.shape[0]} sources but {pb.shape[0]} targets")
    if int(ln.sum()) != int(points.shape[0]):
        raise ValueError(f"pair_stats: lengths sum to {int(ln.sum())}, points holds {int(points.shape[0])} rows")
    Cn, P, dev = int(ln.shape[0]), int(pa.shape[0]), points.device
    T = _dev(T, torch.float64, "pair_stats.T").reshape(P, 4, 4)
    ok = (pa >= 0) & (pa < Cn)
    rows = int(ln[pa[ok]].astype(np.int64).sum())
    matched = torch.zeros((P,), dtype=torch.int32, device=dev)
    moments = torch.zeros((P, 10), dtype=torch.float64, device=dev)
    nn = torch.empty((max(rows, 1),), dtype=torch.int32, device=dev) if correspondences else None
    nbytes = max(L.buf_pair_stats_ws_bytes(int(points.shape[0]), max(Cn, 1), max(P, 1), rows, int(cells_per_elem)), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_pair_stats(_ptr(points), _hptr(ln), Cn, _hptr(pa), _hptr(pb), P, _ptr(T), float(radius), int(cells_per_elem),
                           _ptr(matched), _ptr(moments), _ptr(nn), _ptr(ws), nbytes, _stream()), "buf_pair_stats")
    return matched, moments, (nn[:rows] if nn is not None else None)


PG_MAX_NODES = 128                                                                             # BUF_PG_MAX_NODES
PG_STATUS = ('NOTHING', 'CONVERGED_STEP', 'CONVERGED_COST', 'MAX_ITER', 'STALLED', 'FAILED')   # BUF_PG_* of buffer_hip.h
PG_TICK_HZ = 1e8                                                                               # wall_clock64: a constant 100 MHz


def pose_graph_optimize(nodes, edges, edge_i, edge_j, Z, info, uncertain, fixed, mu, X_init, max_iterations=100, eps_step=1e-9,
                        eps_cost=1e-10, tau0=1e-5, want_ticks=False):
    """buf_pose_graph_optimize: G pose graphs in one launch, nothing read back.  nodes / edges host int[G] (graph g owns nodes[g]
    consecutive poses and edges[g] consecutive edges), edge_i / edge_j host int[E] (graph-local node ids), Z f64[E,4,4] and info
    f64[E,6,6] (device), uncertain host u8[E], fixed host int[G], mu host f64[G], X_init f64[N,4,4] (device)
    -> (X f64[N,4,4], status int32[G,3] = (index into PG_STATUS, solves, accepted), cost f64[G,2] = (initial, final),
    edge f64[E,2] = (l_e, q_e) at X), all on the device; with want_ticks also int64[G,4]: the kernel's own 100 MHz tick counts of
    (everything after the input check, factorisations, substitutions, linearisations + assemblies) per graph."""
    L = _lib.lib()
    nd, ed, fx = _host_i32(nodes), _host_i32(edges), _host_i32(fixed)
    ei, ej = _host_i32(edge_i), _host_i32(edge_j)
    un = np.ascontiguousarray(uncertain, dtype=np.uint8).reshape(-1)
    mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
    G = int(nd.shape[0])
    if not (ed.shape[0] == G and fx.shape[0] == G and mu.shape[0] == G):
        raise ValueError(f"pose_graph_optimize: {G} graphs but {ed.shape[0]} edge counts, {fx.shape[0]} fixed nodes, {mu.shape[0]} weights")
    if (nd < 0).any() or (ed < 0).any():
        raise ValueError("pose_graph_optimize: negative node or edge count")
    N, E = int(nd.astype(np.int64).sum()), int(ed.astype(np.int64).sum())
    if not (ei.shape[0] == E and ej.shape[0] == E and un.shape[0] == E):
        raise ValueError(f"pose_graph_optimize: {E} edges but {ei.shape[0]} / {ej.shape[0]} node ids, {un.shape[0]} flags")
    X_init = _dev(X_init, torch.float64, "pose_graph_optimize.X_init").reshape(N, 4, 4)
    dev = X_init.device
    Z = _dev(Z, torch.float64, "pose_graph_optimize.Z").reshape(E, 4, 4)
    info = _dev(info, torch.float64, "pose_graph_optimize.info").reshape(E, 6, 6)
    X = torch.empty((N, 4, 4), dtype=torch.float64, device=dev)
    status = torch.zeros((G, 3), dtype=torch.int32, device=dev)
    cost = torch.zeros((G, 2), dtype=torch.float64, device=dev)
    edge = torch.zeros((E, 2), dtype=torch.float64, device=dev)
    nbytes = max(L.buf_pose_graph_ws_bytes(max(G, 1), N, E, min(int(nd.max()) if G else 0, PG_MAX_NODES)), 1)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    check(L.buf_pose_graph_optimize(_hptr(nd), _hptr(ed), G, _hptr(ei), _hptr(ej), _ptr(Z), _ptr(info), _hptr(un), _hptr(fx), _hptr(mu),
                                    _ptr(X_init), int(max_iterations), float(eps_step), float(eps_cost), float(tau0), _ptr(X), _ptr(status),
                                    _ptr(cost), _ptr(edge), _ptr(ws), nbytes, _stream()), "buf_pose_graph_optimize")
    if want_ticks:
        return X, status, cost, edge, ws[:32 * G].view(torch.int64).reshape(G, 4).clone()
    return X, status, cost, edge


METRIC_COLUMNS = ('rep_src', 'rep_tgt', 'nn_inl', 'mutual', 'mutual_inl', 'cons', 'cons_true')      # BUF_METRICS_* of buffer_hip.h


def match_metrics(kp, s_nn, t_nn, T_gt, T_est, tau_kp, tau_match, dist_th, want_d2=False):
    """buf_match_metrics: the per-stage ground-truth counts of B pairs in one launch, nothing read back.
    kp f32[2*B*P,3] (pair b: source rows [2bP, 2bP+P), target rows [(2b+1)P, (2b+2)P)), s_nn / t_nn int[B,P] descriptor-space 1-NN
    (source -> target row and the reverse), T_gt [B,4,4] (taken as f64), T_est [B,4,4] (f32) -> counts int32[B,7] on the device,
    columns METRIC_COLUMNS; with want_d2 also f32[2*B*P], the squared distance of every keypoint to the nearest keypoint of the
    pair's other cloud under the ground truth."""
    L = _lib.lib()
    kp = _dev(kp, torch.float32, "match_metrics.kp")
    s_nn, t_nn = _dev(s_nn, torch.int32, "match_metrics.s_nn"), _dev(t_nn, torch.int32, "match_metrics.t_nn")
    if s_nn.dim() != 2 or s_nn.shape != t_nn.shape:
        raise ValueError(f"match_metrics: s_nn {tuple(s_nn.shape)} and t_nn {tuple(t_nn.shape)} must both be [B,P]")
    B, P = int(s_nn.shape[0]), int(s_nn.shape[1])
    if kp.dim() != 2 or tuple(kp.shape) != (2 * B * P, 3):
        raise ValueError(f"match_metrics: kp {tuple(kp.shape)} is not [2*{B}*{P},3]")
    dev = kp.device
    T_gt = torch.as_tensor(T_gt, dtype=torch.float64).to(dev).reshape(B, 4, 4).contiguous()
    T_est = _dev(T_est, torch.float32, "match_metrics.T_est").reshape(B, 4, 4).contiguous()
    counts = torch.empty((B, len(METRIC_COLUMNS)), dtype=torch.int32, device=dev)
    d2 = torch.empty((2 * B * P,), dtype=torch.float32, device=dev) if want_d2 else None
    check(L.buf_match_metrics(_ptr(kp), _ptr(s_nn), _ptr(t_nn), B, P, _ptr(T_gt), _ptr(T_est), float(tau_kp), float(tau_match),
                              float(dist_th), _ptr(counts), _ptr(d2), _stream()), "buf_match_metrics")
    return (counts, d2) if want_d2 else counts


def recover_poses_batched(ind, ss_kpts, tt_kpts, ss_R, tt_R, seg_lengths, seeds, cfg):
    """hypotheses + scoring + RANSAC + refinement of every pair of a step in one set of launches: the matches of the pairs are
    stacked, pair p owns seg_lengths[p] consecutive rows -> poses f32[nb,4,4] (identity for pairs with fewer than 3 matches)."""
    L = _lib.lib()
    seg = _host_i32(seg_lengths)
    nb, M = int(seg.shape[0]), int(seg.sum())
    dev = ss_kpts.device
    poses = torch.empty((nb, 4, 4), dtype=torch.float32, device=dev)
    if nb == 0:
        return poses
    nbytes = L.buf_recover_poses_ws_bytes(M, nb, int(cfg.ransac_hypotheses))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sd = (C.c_ulonglong * nb)(*[int(x) & _MASK64 for x in seeds])
    check(L.buf_recover_poses_batched(_ptr(ind.contiguous()), _ptr(ss_kpts.contiguous()), _ptr(tt_kpts.contiguous()),
                                      _ptr(ss_R.contiguous()), _ptr(tt_R.contiguous()), _hptr(seg), nb, sd, int(cfg.azi_n),
                                      float(cfg.inlier_th), int(cfg.ransac_hypotheses), float(cfg.dist_th), float(cfg.similar_th),
                                      float(cfg.refine_threshold), 20 if cfg.pose_refine else 0, _ptr(poses), _ptr(ws), nbytes,
                                      _stream()), "buf_recover_poses_batched")
    return poses


# ----------------------------------------------------------------------------- fused descriptor CNN
def mfma_tile_weights(wt, lk_major=False):
    """[K, Cout] (K, Cout multiples of 16) -> the B-operand tiling of the fused MFMA kernels: blocks [K/16][Cout/16] of
    256 floats laid out [lk][li][p], so that a lane's four k-steps are one 16-byte load.  K-row of (g, p, lk):
    16g + 4p + lk (k-step p takes channels 4p..4p+3: csrc/convnet.hip), or with lk_major 16g + 4lk + p (k-step p takes
    channel 4lk + p of every lane quarter, the order of csrc/costnet.hip's 16-byte A-fragment loads)."""
    K, cout = wt.shape
    assert K % 16 == 0 and cout % 16 == 0
    t = wt.reshape(K // 16, 4, 4, cout // 16, 16)            # [g, p, lk, n, li]  or  [g, lk, p, n, li]
    perm = (0, 3, 1, 4, 2) if lk_major else (0, 3, 2, 4, 1)
    return np.ascontiguousarray(np.transpose(t, perm), dtype=np.float32).reshape(-1)              # [g, n, lk, li, p]


def winograd_tile_weights(w, ng=None, blocks=4):
    """[Cout, Cin, 3, 3] -> the F(2x2, 3x3) filter transform U = G g G^T (fp64, rounded once to fp32) in the A-operand tiling
    of csrc/convnet_wg.hip: [N-group][i][k-step][n2][lk][li][j] = U[i][j][16 (NG g + n2) + li][4 ks + lk], N-groups of NG = 2
    N-tiles (a wavefront owns an N-tile pair in every layer).  16 * Cout * Cin floats (buf_winograd_tile_weights is the same function
    on the C side).  ng / blocks: the general form (buf_winograd_tile_filters); blocks = 5 appends g[1] G^T = U_1 - U_2."""
    cout, cin = w.shape[0], w.shape[1]
    assert cin % 4 == 0 and cout % 16 == 0
    if ng is None:
        ng = _lib.lib().buf_winograd_group(cin, cout)              # N-tiles per wavefront for these widths: the kernel's rule
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
    G5 = np.concatenate([G, [[0, 1, 0]]])                                              # row 4: the filter's middle row as it is
    U = np.einsum('ia,ocab,jb->ijoc', G5, np.asarray(w, np.float64), G)                # [i, j, Cout, Cin]
    U = U[:blocks].reshape(blocks, 4, cout // (16 * ng), ng, 16, cin // 4, 4)          # [i, j, g, n2, li, ks, lk]
    return np.ascontiguousarray(np.transpose(U, (2, 0, 5, 3, 6, 4, 1)), dtype=np.float32).reshape(-1)


def winograd_f24_tile_weights(w):
    """[Cout, Cin, 3, 3] -> the F(2x4, 3x3) filter transform U = G2 g G4^T (fp64, rounded once to fp32; points 0, +-1, +-2, infinity
    along the azimuth) in the tiling of csrc/convnet_w24.hip: [pair][i][k-step][768] with, per (row component i, k-step), the column
    components j = 0, 1, 2, 5 of both N-tiles as [n2][lk][li][4] and then j = 3, 4 as [n2][lk][li][2]; value
    U[i][j][16 (2 pair + n2) + li][4 ks + lk].  24 * Cout * Cin floats, bit for bit what buf_winograd_f24_tile_weights writes (the
    nine products are summed in its order)."""
    cout, cin = w.shape[0], w.shape[1]
    assert cin % 4 == 0 and cout % 32 == 0
    U = winograd_f24_filters(w)
    U = U.reshape(4, 6, cout // 32, 2, 16, cin // 4, 4)                              # [i, j, pair, n2, li, ks, lk]
    U = np.transpose(U, (2, 0, 5, 3, 6, 4, 1))                                       # [pair, i, ks, n2, lk, li, j]
    lead = U.shape[:3]
    wide = U[..., [0, 1, 2, 5]].reshape(*lead, 512)
    narrow = U[..., [3, 4]].reshape(*lead, 256)
    return np.ascontiguousarray(np.concatenate([wide, narrow], axis=-1), dtype=np.float32).reshape(-1)


F24_G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
F24_G4 = np.array([[.25, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                  np.float64)


def winograd_f24_filters(w):
    """[Cout, Cin, 3, 3] -> U = G2 g G4^T in float64, [4, 6, Cout, Cin]"""
    w64 = np.asarray(w, np.float64)
    U = np.zeros((4, 6) + w64.shape[:2], np.float64)
    for a in range(3):
        for b in range(3):
            U += (F24_G2[:, a][:, None, None, None] * w64[None, None, :, :, a, b]) * F24_G4[:, b][None, :, None, None]
    return U


# F(2x5, 3x3): F(2,3) down the rows as above, F(5,3) along the azimuth on the seven points 0, +-1, +-2, +-1/2 (no point at infinity: the
# product polynomial has degree 6).  Column component j belongs to point F25_POINTS[j]; B5^T row j holds the coefficients of
# L_j(x) = prod_{k != j} (x - p_k), G5 row j the powers of p_j over L_j(p_j), A5^T row i the i-th powers of the points.
F25_POINTS = (0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5)


def _f25_matrices():
    pts = np.array(F25_POINTS, np.float64)
    bt = np.zeros((7, 7))
    g = np.zeros((7, 3))
    for j, p in enumerate(pts):
        lj = np.poly(np.delete(pts, j))[::-1]                                        # ascending powers, monic
        bt[j] = lj
        nj = np.prod(p - np.delete(pts, j))                                          # L_j(p_j), exact in float64
        g[j] = [1 / nj, p / nj, p * p / nj]
    at = pts[None, :] ** np.arange(5)[:, None]
    return np.round(bt * 16) / 16, g, at                                             # (the coefficients of L_j are multiples of 1/16)


F25_B5T, F25_G5, F25_A5T = _f25_matrices()


def winograd_f25_filters(w):
    """[Cout, Cin, 3, 3] -> U = G2 g G5^T in float64, [4, 7, Cout, Cin]"""
    w64 = np.asarray(w, np.float64)
    U = np.zeros((4, 7) + w64.shape[:2], np.float64)
    for a in range(3):
        for b in range(3):
            U += (F24_G2[:, a][:, None, None, None] * w64[None, None, :, :, a, b]) * F25_G5[:, b][None, :, None, None]
    return U


def winograd_f25_tile_weights(w):
    """[Cout, Cin, 3, 3] -> the F(2x5, 3x3) filter transform U = G2 g G5^T (fp64, rounded once to fp32) in the tiling of
    csrc/convnet_w25.hip: [i][k-step][N-tile][448] with, per (row component i, k-step, N-tile), the column components j = 0..3 as
    [lk][li][4], then j = 4, 5 as [lk][li][2], then j = 6 as [lk][li]; value U[i][j][16 n + li][4 ks + lk].  28 * Cout * Cin floats
    (buf_winograd_f25_tile_weights is the same function on the C side)."""
    cout, cin = w.shape[0], w.shape[1]
    assert cin % 4 == 0 and cout % 16 == 0
    U = winograd_f25_filters(w).reshape(4, 7, cout // 16, 16, cin // 4, 4)           # [i, j, n, li, ks, lk]
    U = np.transpose(U, (0, 4, 2, 5, 3, 1))                                          # [i, ks, n, lk, li, j]
    lead = U.shape[:3]
    parts = [U[..., 0:4].reshape(*lead, 256), U[..., 4:6].reshape(*lead, 128), U[..., 6:7].reshape(*lead, 64)]
    return np.ascontiguousarray(np.concatenate(parts, axis=-1), dtype=np.float32).reshape(-1)


F24_FLAG = 2          # relu_host[l] bit 1 of buf_cylindrical_net_wg: the layer's buffer holds the F(2x4) set behind the F(2x2) set
F24K_FLAG = 4         # bit 2: the same for a layer with 64 output channels and Cin % 64 == 0 (K split or pass split, as the call's form says)
F24P_DEFAULT = True   # the form of the bit-2 layers: pass split (csrc/convnet_w24p.hip) | K split (csrc/convnet_w24k.hip); profiles/f24p_ab.md
# F(2x4) sets of the layers' own (csrc/convnet_w24a.hip; profiles/f24a_ab.md): F(2x4) tiles in 'all' layers; 'out64': only in the
# 64-output layers the flags leave in the F(2x2) form (the released stack: layer 0); 'out32': only in the 32-output layers; 'off' or
# None: those layers stay in the F(2x2) form.  The argument f24a= of the two classes picks one per net.
F24A_DEFAULT = 'all'
F24A_PARTS = {'all': (64, 32), 'out64': (64,), 'out32': (32,), 'off': (), None: ()}


# F(2x5) tiles (csrc/convnet_w25.hip; profiles/f25_ab.md): the layers of these output widths run on an F(2x5) set of their
# own -- 'all': the 64- and the 32-output layers, 'out64' / 'out32': one of the two, 'off' or None: no such layer, the other forms' bits.
# The 128-output form ('out128') is not built.  The argument f25= of the two classes picks one per net.  The default is the part that met
# both rules of the A/B (profiles/f25_ab.md): the 64-output layers; the 32-output form measured slower than its F(2x4) twin and stays off.
F25_DEFAULT = 'out64'
F25_PARTS = {'all': (64, 32), 'out64': (64,), 'out32': (32,), 'off': (), None: ()}


def form_parts(name, value, default, table):
    """What a form argument of the four net classes names in `table`: None -> `default`, True -> 'all', False -> 'off', else a key."""
    value = default if value is None else 'all' if value is True else 'off' if value is False else value
    if value not in table:
        raise ValueError(f"{name} = {value!r}: one of " + ", ".join(repr(k) for k in table if k is not None))
    return table[value]


# Row 6 of the 128-output layers (csrc/convnet_w25t.hip; profiles/cyl_taps_ab.md): 'taps': the direct round of output row 6
# runs on the filter rows 0 and 1 as the host tiled them (a set of 6 Cout Cin floats per layer) instead of forming its taps per patch from
# three Winograd block rows; 'order': the direct round runs in front of the Winograd round, whose 64 outputs per lane then need no parking;
# 'both' (or 'all'); 'off' or None: the 128-output layers as the other arguments leave them, bit for bit.  The argument row6= of the two classes
# picks one per net; a net built with any other form argument keeps its layer forms as they were unless row6= asks.  The default is what met both
# rules of the A/B (profiles/cyl_taps_ab.md): both parts together.
ROW6_DEFAULT = 'both'
ROW6_PARTS = {'both': (True, True), 'all': (True, True), 'taps': (True, False), 'order': (False, True), 'off': (False, False), None: (False, False)}


def cyl_row6_tile_taps(w):
    """[Cout, Cin, 3, 3] -> the six taps of output row 6, the filter rows a = 0, 1 as they are, in the tiling of csrc/convnet_w25t.hip:
    [pair][k-step][q = 0..2][lk][li][4] with float 4 q + e = 6 n2 + 3 a + b of lane (lk, li) = w[16 (2 pair + n2) + li][4 ks + lk][a][b].
    6 * Cout * Cin floats, bit for bit what buf_cyl_row6_tile_taps writes."""
    cout, cin = w.shape[0], w.shape[1]
    assert cin % 4 == 0 and cout % 32 == 0
    t = np.asarray(w, np.float32)[:, :, :2, :].reshape(cout // 32, 2, 16, cin // 4, 4, 6)      # [pair, n2, li, ks, lk, (a, b)]
    t = np.transpose(t, (0, 3, 4, 2, 1, 5)).reshape(cout // 32, cin // 4, 4, 16, 3, 4)           # [pair, ks, lk, li, q, e]
    return np.ascontiguousarray(np.transpose(t, (0, 1, 4, 2, 3, 5))).reshape(-1)                # [pair, ks, q, lk, li, e]


def cyl_layer_filters(w, f24k=True):
    """The fp32 kernel's filter buffer of one layer and its F(2x4) flag: layers with 128 output channels run in the F(2x4) form
    (flag 2) and, with f24k, so do the layers with 64 output channels whose Cin is a multiple of 64 (flag 4: K split or pass split,
    as the call's form says); both carry that set behind the F(2x2) one."""
    wt = winograd_tile_weights(w)
    cout, cin = w.shape[0], w.shape[1]
    if cout == 128:
        flag = F24_FLAG
    elif f24k and cout == 64 and cin % 64 == 0:
        flag = F24K_FLAG
    else:
        return wt, 0
    return np.concatenate([wt, winograd_f24_tile_weights(w)]), flag


def cyl_forms(f24, f24k, f24p, f24a, f25, row6):
    """The form arguments of the two net classes, resolved once -> (f24, f24k, f24p with their defaults filled in, the output widths
    whose unflagged layers get an F(2x4) set of their own, the output widths whose layers get an F(2x5) set, (taps, order first) of the
    128-output layers).  An explicit older argument switches the newer defaults off: f24 / f24k / f24p those of f24a and f25, any of the
    five that of row6.  Asking for a newer form with f24, f24k or f24p false is an error."""
    older = not (f24 is None and f24k is None and f24p is None)
    kept = f24 in (None, True) and f24k in (None, True) and f24p in (None, True)
    if f25 == 'out128':
        raise ValueError("f25 = 'out128': the 128-output layers have no F(2x5) form (csrc/convnet_w25.hip)")
    parts = {}
    for name, value, default, table in (('f25', f25, None if older else F25_DEFAULT, F25_PARTS),
                                        ('row6', row6, None if older or f24a is not None or f25 is not None else ROW6_DEFAULT, ROW6_PARTS),
                                        ('f24a', f24a, None if older else F24A_DEFAULT, F24A_PARTS)):
        parts[name] = form_parts(name, value, default, table)
        if any(parts[name]) and not kept:
            raise ValueError(name + " goes with the default forms of the other layers (f24, f24k, f24p left alone or true)")
    f24, f24k, f24p = (True if f24 is None else f24), (True if f24k is None else f24k), (F24P_DEFAULT if f24p is None else f24p)
    return f24, f24k, f24p, parts['f24a'], parts['f25'], parts['row6']


def cyl_own_sets(layers, flags, takes, tiler, device):
    """Per layer `tiler(w)` in a buffer of its own (a tensor on `device`) where `takes(w, flag)`, else None; and the pointer array the
    entry points with sets take."""
    sets = [torch.from_numpy(tiler(w)).to(device) if takes(w, flag) else None for (w, _, _), flag in zip(layers, flags)]
    return sets, (C.c_void_p * len(sets))(*[None if t is None else t.data_ptr() for t in sets])


class CylindricalNet:
    """Device weights of Cylindrical_Net for the fused fp32 kernels (csrc/convnet_w*.hip): per layer U = G g G^T in the kernel's tiling
    (layers flagged for the F(2x4) form: that set behind it, flagged in the relu word), the sets of the layers' own in buffers of their
    own (`wt24`: F(2x4), `wt25`: F(2x5), `taps`: row 6), biases."""

    def __init__(self, layers, device, f24=None, f24k=None, f24p=None, f24a=None, f25=None, row6=None):
        """layers: list of 8 (w [Cout,Cin,3,3] np.float32 with BN folded, b [Cout], relu).  Each argument selects a layer form; no form
        argument: every default below.
        f24 (True): the 128-output layers on F(2x4) tiles; False: the F(2x2) form in every layer (the cross-check of the tests and the
        A side of an A/B).
        f24k (True): the 64-output layers with Cin % 64 == 0 on F(2x4) tiles as well; False: F(2x4) in the 128-output layers only.
        f24p (F24P_DEFAULT): those 64-output layers in the pass-split form, else K split.
        f24a = 'all' | 'out64' | 'out32' | 'off' (F24A_DEFAULT): F(2x4) sets of their own for the remaining layers of those output
        widths.
        f25 = 'all' | 'out64' | 'out32' | 'off' (F25_DEFAULT): F(2x5) tiles in the layers of those output widths; the other layers as
        the remaining arguments say.
        row6 = 'both' | 'taps' | 'order' | 'off' (ROW6_DEFAULT): host-formed row-6 taps and / or the direct round first in the
        128-output layers.
        An explicit older argument switches the defaults of the newer ones off (cyl_forms)."""
        f24, f24k, f24p, parts, parts25, (row6_taps, row6_first) = cyl_forms(f24, f24k, f24p, f24a, f25, row6)
        self.wt, self.bias, self.cin, self.cout, self.relu = [], [], [], [], []
        self.entry = "buf_cylindrical_net_wg"            # the family (CylindricalNetSplit: "buf_cylindrical_net_split"); self.fn is what is called
        self.form = 1 if f24p else 0
        flags = []
        for w, b, relu in layers:
            cout, cin = w.shape[0], w.shape[1]
            wt, flag = cyl_layer_filters(w, f24k) if f24 else (winograd_tile_weights(w), 0)
            flags.append(flag)
            self.wt.append(torch.from_numpy(wt).to(device))
            self.bias.append(torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(device))
            self.cin.append(cin); self.cout.append(cout); self.relu.append(1 if relu else 0)
        n = len(layers)
        self._wp = (C.c_void_p * n)(*[t.data_ptr() for t in self.wt])
        self._bp = (C.c_void_p * n)(*[t.data_ptr() for t in self.bias])
        self._ci = (C.c_int * n)(*self.cin)
        self._co = (C.c_int * n)(*self.cout)
        self._re = (C.c_int * n)(*[r | f for r, f in zip(self.relu, flags)])
        small = lambda w: w.shape[0] in (32, 64) and w.shape[1] % 16 == 0
        # the unflagged layers that run on an F(2x4) set of their own; f24_all: every layer of the stack runs on F(2x4) tiles
        self.wt24, self._w24p = cyl_own_sets(layers, flags, lambda w, flag: flag == 0 and w.shape[0] in parts and small(w),
                                             winograd_f24_tile_weights, device)
        self.f24_layers = [l for l, t in enumerate(self.wt24) if t is not None]
        self.f24_all = bool(self.f24_layers) and all(f or t is not None for f, t in zip(flags, self.wt24))
        # the layers that run on an F(2x5) set (it wins over the layer's F(2x4) flag or set)
        self.wt25, self._w25p = cyl_own_sets(layers, flags, lambda w, flag: w.shape[0] in parts25 and small(w), winograd_f25_tile_weights, device)
        self.f25_layers = [l for l, t in enumerate(self.wt25) if t is not None]
        # the 128-output layers that run on a row-6 tap set, and the order of their two rounds
        self.taps, self._tapsp = cyl_own_sets(layers, flags, lambda w, flag: row6_taps and flag == F24_FLAG, cyl_row6_tile_taps, device)
        self.taps_layers = [l for l, t in enumerate(self.taps) if t is not None]
        self.row6_first = bool(row6_first and F24_FLAG in flags)
        # The entry point, chosen once: the fp32 call, the split-safe call of CylindricalNetSplit, and what both take between the relu
        # words and the outputs
        if self.taps_layers or self.row6_first:
            fn, safe, self._extra = "w25t", "split_safe_w25t", (self._w24p, self._w25p, self._tapsp, 1 if self.row6_first else 0)
        elif self.f25_layers:
            fn, safe, self._extra = "w25", "split_safe_w25", (self._w24p, self._w25p)
        elif self.f24_layers:
            fn, safe, self._extra = "wg_all", "split_safe_all", (self._w24p,)
        else:
            fn, safe, self._extra = "wg_form", "split_safe_form", (self.form,)
        self.fn, self.fn_split_safe = "buf_cylindrical_net_" + fn, "buf_cylindrical_net_" + safe

    def __call__(self, x):
        """x f32[P,16,420] (or [P,48,140]) -> f32[P,32,7,20]"""
        x = x.contiguous()
        P = x.shape[0]
        y = torch.empty((P, self.cout[-1], 7, 20), dtype=torch.float32, device=x.device)
        check(getattr(_lib.lib(), self.fn)(_ptr(x), P, self._wp, self._bp, self._ci, self._co, self._re, *self._extra, _ptr(y), _stream()), self.fn)
        return y


def split_tile_filters(w):
    """[Cout, Cin, 3, 3] fp32 -> the two f16 planes of csrc/convnet_h3.hip (hi = f16(w), lo' = f16((w - hi) 2^11)) in the kernel's
    tiling, as uint16 bit patterns (buf_split_tile_filters; host only)."""
    L = _lib.lib()
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin = w.shape[0], w.shape[1]
    out = np.empty(L.buf_split_filter_count(cout, cin), dtype=np.uint16)
    check(L.buf_split_tile_filters(w.ctypes.data, cout, cin, out.ctypes.data), "buf_split_tile_filters")
    return out


class CylindricalNetSplit:
    """Cylindrical_Net on the f16 matrix pipe with fp32-equivalent arithmetic (csrc/convnet_h3.hip, "split-f16"): opt-in next to
    CylindricalNet.  Same call, same [P,32,7,20] fp32 result to fp32 round-off.

    Safe by construction (round 6, csrc/split_safe.hip): the kernel flags every patch whose input or hidden activation leaves the f16
    range (|v| >= 65504, NaN included) and the fp32 kernel of CylindricalNet re-runs exactly those patches in the same stream, masked by
    the flags -- no host round trip, no exception; `last_flags` (int32[P], device) marks the patches of the last call that took the fp32
    kernel.  For widths the fp32 kernel is not built for (the released network's are) the old contract stays: `check_range()` raises if
    the status word was set."""

    def __init__(self, layers, device, f24k=None, f24p=None, f24a=None, f25=None, row6=None):
        """f24k, f24p, f24a, f25, row6: the layer forms of the fp32 re-run, as in CylindricalNet"""
        form = cyl_forms(None, f24k, f24p, f24a, f25, row6)[2]       # (the arguments are checked whether or not the fp32 side gets built)
        self.wt, self.bias, self.cin, self.cout, self.relu = [], [], [], [], []
        self.entry = "buf_cylindrical_net_split"
        self.f24_layers, self.f24_all, self.f25_layers, self.taps_layers, self.row6_first = [], False, [], [], False
        self.form = 1 if form else 0                     # of the fp32 re-run, as in CylindricalNet
        for w, b, relu in layers:
            cout, cin = w.shape[0], w.shape[1]
            self.wt.append(torch.from_numpy(split_tile_filters(w).view(np.int16)).to(device))
            self.bias.append(torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(device))
            self.cin.append(cin); self.cout.append(cout); self.relu.append(1 if relu else 0)
        n = len(layers)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._wp = (C.c_void_p * n)(*[t.data_ptr() for t in self.wt])
        self._bp = (C.c_void_p * n)(*[t.data_ptr() for t in self.bias])
        self._ci = (C.c_int * n)(*self.cin)
        self._co = (C.c_int * n)(*self.cout)
        self._re = (C.c_int * n)(*self.relu)
        self.last_flags = None
        # the fp32 re-run is a CylindricalNet over the same layers (the split kernel itself takes the relu words 0 / 1); widths it is not
        # built for keep the raising contract
        self.safe = n == 8 and _lib.lib().buf_cylindrical_net_wg_supports(self._ci, self._co) == 0 and not os.environ.get('BUF_SPLIT_UNSAFE')
        self.f32 = CylindricalNet(layers, device, f24k=f24k, f24p=f24p, f24a=f24a, f25=f25, row6=row6) if self.safe else None
        if self.safe:
            f = self.f32
            self.wt_wg, self._wwp, self._re_safe = f.wt, f._wp, f._re
            self.wt24, self._w24p, self.f24_layers, self.f24_all = f.wt24, f._w24p, f.f24_layers, f.f24_all
            self.wt25, self._w25p, self.f25_layers = f.wt25, f._w25p, f.f25_layers
            self.taps, self._tapsp, self.taps_layers, self.row6_first = f.taps, f._tapsp, f.taps_layers, f.row6_first
            self.fn = f.fn_split_safe

    def _safe_call(self, x, head):
        x = x.contiguous()
        P = x.shape[0]
        out = torch.empty((P, self.cout[-1], 7, 20), dtype=torch.float32, device=x.device)
        desc = torch.empty((P, 32), dtype=torch.float32, device=x.device) if head is not None else None
        self.last_flags = torch.empty((max(P, 1),), dtype=torch.int32, device=x.device)
        check(getattr(_lib.lib(), self.fn)(_ptr(x), P, self._wp, self._wwp, self._bp, self._ci, self._co, self._re_safe, *self.f32._extra,
                                           _ptr(head.params) if head is not None else None, _ptr(out), _ptr(desc), _ptr(self.status),
                                           _ptr(self.last_flags), _stream()), self.fn)
        return (desc, out) if head is not None else out

    def __call__(self, x):
        """x f32[P,16,420] (or [P,48,140]) -> f32[P,32,7,20]"""
        if self.safe:
            return self._safe_call(x, None)
        L = _lib.lib()
        x = x.contiguous()
        P = x.shape[0]
        y = torch.empty((P, self.cout[-1], 7, 20), dtype=torch.float32, device=x.device)
        check(L.buf_cylindrical_net_split(_ptr(x), P, self._wp, self._bp, self._ci, self._co, self._re, _ptr(y), _ptr(self.status), _stream()),
              self.entry)
        return y

    def with_head(self, x, head):
        """x f32[P,16,420] -> (desc f32[P,32], equi f32[P,32,7,20]) with DescriptorHead `head` fused behind the last layer: the
        [32][140] map never leaves LDS; bit-identical to head(self(x))."""
        if self.safe:
            return self._safe_call(x, head)
        L = _lib.lib()
        x = x.contiguous()
        P = x.shape[0]
        desc = torch.empty((P, 32), dtype=torch.float32, device=x.device)
        equi = torch.empty((P, 32, 7, 20), dtype=torch.float32, device=x.device)
        check(L.buf_cylindrical_net_split_head(_ptr(x), P, self._wp, self._bp, self._ci, self._co, self._re, _ptr(head.params),
                                               _ptr(desc), _ptr(equi), _ptr(self.status), _stream()), "buf_cylindrical_net_split_head")
        return desc, equi

    def range_fallbacks(self):
        """patches of the last call that left the f16 range and were recomputed by the fp32 kernel (reads the flags: synchronises)"""
        return 0 if self.last_flags is None else int((self.last_flags != 0).sum().item())

    def check_range(self):
        """Safe form: nothing to raise (flagged patches were recomputed in fp32); clears the informational status word.  Otherwise
        (widths without an fp32 kernel): raises FloatingPointError if an activation left the f16 range."""
        if int(self.status.item()) != 0:
            self.status.zero_()
            if not self.safe:
                raise FloatingPointError("buf_cylindrical_net_split: an activation left the f16 range (|v| >= 65504); use the fp32 kernel")


class DescriptorHead:
    """Attention pooling + normalisation head (patch_embedder.py:66-72,81-84) for csrc/convnet.hip k_desc_head."""

    def __init__(self, w0, b0, w3, b3, device):
        """w0 [16,32], b0 [16], w3 [16], b3 [1]: np.float32, BatchNorms folded -> one device parameter block"""
        f = lambda a, n: np.asarray(a, dtype=np.float32).reshape(n)
        self.params = torch.from_numpy(np.concatenate([f(w0, 512), f(b0, 16), f(w3, 16), f(b3, 1)])).to(device)

    def __call__(self, y):
        """y f32[P,32,7,20] -> desc f32[P,32], equi f32[P,32,7,20]"""
        L = _lib.lib()
        y = y.contiguous()
        P = y.shape[0]
        assert y.dtype == torch.float32 and y.numel() == P * 32 * 140
        desc = torch.empty((P, 32), dtype=torch.float32, device=y.device)
        equi = torch.empty((P, 32, 7, 20), dtype=torch.float32, device=y.device)
        check(L.buf_descriptor_head(_ptr(y), P, _ptr(self.params), _ptr(desc), _ptr(equi), _stream()), "buf_descriptor_head")
        return desc, equi


def split_tile_gemm(w, nt):
    """[Cout, Cin, ntaps] fp32 -> the two f16 planes (hi, lo') in the tiling of csrc/costnet_h3.hip's ch_gemm, groups of nt
    16-output tiles, as uint16 bit patterns (buf_split_tile_gemm; host only)."""
    L = _lib.lib()
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin, ntaps = w.shape
    out = np.empty(L.buf_split_gemm_count(cout, cin, ntaps, nt), dtype=np.uint16)
    check(L.buf_split_tile_gemm(w.ctypes.data, cout, cin, ntaps, nt, out.ctypes.data), "buf_split_tile_gemm")
    return out


def separate_cost_layer0(w):
    """Layer 0 of CostNet is linear in cost[c][n][k][l] = S[c][k][(l-n) mod 20] - T[c][k][l] (models/BUFFER.py:49-60), so its
    3x3x3 kernel w [32,32,3(dn),3(dk),3(dl)] separates exactly into a kernel on S indexed by e = dl - dn (the S-term of an
    output depends on (k', (l'-n') mod 20) only) and one on T summed over dn (the T-term does not depend on n'):
      Ws[(dk*5 + e+2)*32 + c][o] = sum_{dl-dn=e} w[o][c][dn][dk][dl],   Wt[(dk*3 + dl)*32 + c][o] = sum_dn w[o][c][dn][dk][dl]
    (fp64 sums, fp32 storage) -> (Ws f32[480,32], Wt f32[288,32])."""
    w = np.asarray(w, np.float64)
    cout, cin = w.shape[0], w.shape[1]
    ws = np.zeros((3, 5, cin, cout))
    for dn in range(3):
        for dl in range(3):
            ws[:, dl - dn + 2] += np.transpose(w[:, :, dn, :, dl], (2, 1, 0))        # [dk, c, o]
    wt = np.transpose(w.sum(2), (2, 3, 1, 0))                                       # [dk, dl, c, o]
    return ws.reshape(-1, cout).astype(np.float32), wt.reshape(-1, cout).astype(np.float32)


# What a cost net built without a form argument runs (the forms of csrc/costnet_w24.hip; profiles/cost_f24_ab.md): 'all': F(2x4) tiles in
# layers 2 and 4 and the Winograd F(2x2) form in layer 6; 'l2', 'l4', 'l6': one of the three alone; 'off' or None: every layer in its first
# form (F(2x2) in layers 1..5, layer 6 direct), bit for bit.  The argument f24= of CostVolumeNet, CostVolumeNetSplit and registration.CostVolume picks one per net.
COST_F24_DEFAULT = 'all'
COST_F24_PARTS = {'all': (2, 4, 6), 'l2': (2,), 'l4': (4,), 'l6': (6,), 'off': (), None: ()}


def cost_f24_parts(f24):
    return form_parts('f24', f24, COST_F24_DEFAULT, COST_F24_PARTS)


def cost_f24_filters(layers, parts):
    """The three extra filter sets of the *_w24 entry points (None where the layer keeps its first form): layers 2 and 4 in the F(2x4) tiling
    (winograd_f24_tile_weights of the (3,1,3) filters as [Cout][Cin][3][3]), layer 6 in the F(2x2) tiling with one N-tile per group."""
    sets = []
    for l in (2, 4, 6):
        if l not in parts:
            sets.append(None)
            continue
        w = layers[l][0]
        assert tuple(w.shape[2:]) == (3, 1, 3), w.shape
        w2d = np.ascontiguousarray(w[:, :, :, 0, :])
        sets.append(winograd_tile_weights(w2d, ng=1) if l == 6 else winograd_f24_tile_weights(w2d))
    return sets


# The forms of csrc/costnet_w24b.hip (profiles/cost_f24b_ab.md) beside those above: 'all': layer 1 on F(2x4) tiles and layer 3
# as F(2x4) rows with an F(2x2) tail; 'l1', 'l3': one of the two alone; 'off': layers 1 and 3 in their F(2x2) form, bit for bit.  The
# argument f24b= picks one per net.  Left alone it is COST_F24B_DEFAULT for a net built with no form argument at all, and 'off' beside an
# explicit f24=, which asks for the net as it was before these two forms.
COST_F24B_DEFAULT = 'all'
COST_F24B_PARTS = {'all': (1, 3), 'l1': (1,), 'l3': (3,), 'off': ()}


def cost_f24b_parts(f24, f24b):
    return form_parts('f24b', f24b, COST_F24B_DEFAULT if f24 is None else 'off', COST_F24B_PARTS)


def cost_f24b_filters(layers, parts):
    """The two extra filter sets of the *_w24b entry points (None where the layer keeps its form): winograd_f24_tile_weights of layer 1's collapsed
    filter [64][96 = (dk, c)][dn][dl] and of layer 3's (3,1,3) filter as [128][64][3][3]."""
    sets = []
    for l in (1, 3):
        if l not in parts:
            sets.append(None)
            continue
        w = layers[l][0]
        if l == 1:
            assert tuple(w.shape) == (64, 32, 3, 3, 3), w.shape
            w2d = np.ascontiguousarray(np.transpose(w, (0, 3, 1, 2, 4)).reshape(64, 96, 3, 3))
        else:
            assert tuple(w.shape[2:]) == (3, 1, 3), w.shape
            w2d = np.ascontiguousarray(w[:, :, :, 0, :])
        sets.append(winograd_f24_tile_weights(w2d))
    return sets


class CostVolumeNet:
    """Device weights of CostNet re-laid for csrc/costnet.hip: layer 0 in its separated form (separate_cost_layer0: Ws then
    Wt in one buffer), layers 6..9 as Wt[((dn*KH+dk)*KW+dl)*Cin + c][Cout], MFMA-tiled; layers 1..5 as U = G g G^T in the
    Winograd tiling (winograd_tile_weights; groups per buf_cost_winograd_group; layer 1 with its three k planes as channels).
    f24: the parts that run in the forms of csrc/costnet_w24.hip (COST_F24_DEFAULT); their sets live in buffers of their own (self.wt24).
    f24b: the parts that run in the forms of csrc/costnet_w24b.hip (cost_f24b_parts); their sets: self.wt24b."""

    def __init__(self, layers, device, f24=None, f24b=None):
        """layers: 10 x (w [Cout,Cin,KD,KH,KW] np.float32 with BN folded, b [Cout])"""
        assert len(layers) == 10
        self.parts = cost_f24_parts(f24)
        self.parts_b = cost_f24b_parts(f24, f24b)
        self.wt24 = [None if a is None else torch.from_numpy(a).to(device) for a in cost_f24_filters(layers, self.parts)]
        self._fp = (C.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in self.wt24])
        self.wt24b = [None if a is None else torch.from_numpy(a).to(device) for a in cost_f24b_filters(layers, self.parts_b)]
        self._fpb = (C.c_void_p * 5)(*[None if t is None else t.data_ptr() for t in self.wt24 + self.wt24b])      # the five of the *_w24b entry points
        self.wt, self.bias = [], []
        for i, (w, b) in enumerate(layers):
            cout, cin = w.shape[0], w.shape[1]
            b = np.asarray(b, np.float32)
            if i == 0:
                assert tuple(w.shape) == (32, 32, 3, 3, 3), w.shape
                tiled = np.concatenate([mfma_tile_weights(m, lk_major=True) for m in separate_cost_layer0(w)])
                self.wt.append(torch.from_numpy(tiled).to(device))
                self.bias.append(torch.from_numpy(np.ascontiguousarray(b)).to(device))
                continue
            if i == 1:
                # layer 1 collapses k' (3 -> 1): a 3 x 3 correlation over (n', l') with the three k' planes as input channels
                assert tuple(w.shape) == (64, 32, 3, 3, 3), w.shape
                w2d = np.ascontiguousarray(np.transpose(w, (0, 3, 1, 2, 4)).reshape(64, 96, 3, 3))     # [o][(dk, c)][dn][dl]
                self.wt.append(torch.from_numpy(winograd_tile_weights(w2d, ng=_lib.lib().buf_cost_winograd_group(1))).to(device))
                self.bias.append(torch.from_numpy(np.ascontiguousarray(b)).to(device))
                continue
            if 2 <= i <= 5:                               # the (3,1,3) layers 16 -> 14 -> 12 -> 10 -> 8 run in the Winograd domain
                assert tuple(w.shape[2:]) == (3, 1, 3), w.shape
                tiled = winograd_tile_weights(np.ascontiguousarray(w[:, :, :, 0, :]), ng=_lib.lib().buf_cost_winograd_group(i))
                self.wt.append(torch.from_numpy(tiled).to(device))
                self.bias.append(torch.from_numpy(np.ascontiguousarray(b)).to(device))
                continue
            wt = np.transpose(w, (2, 3, 4, 1, 0)).reshape(-1, cout)
            if i == 9:                                    # 20 logits -> two full 16-column tiles
                wt = np.concatenate([wt, np.zeros((wt.shape[0], 32 - cout), np.float32)], 1)
                b = np.concatenate([b, np.zeros(32 - cout, np.float32)])
            self.wt.append(torch.from_numpy(mfma_tile_weights(np.ascontiguousarray(wt, dtype=np.float32), lk_major=True)).to(device))
            self.bias.append(torch.from_numpy(np.ascontiguousarray(b)).to(device))
        self._wp = (C.c_void_p * 10)(*[t.data_ptr() for t in self.wt])
        self._bp = (C.c_void_p * 10)(*[t.data_ptr() for t in self.bias])
        # The family of entry points, chosen once (one kernel runs all three): the suffix of its dense, gathered and split-safe entry
        # points and the sets they take behind the biases
        if self.parts_b:
            self.kernel, self._sets = "_w24b", (self._fpb,)
        elif self.parts:
            self.kernel, self._sets = "_w24", (self._fp,)
        else:
            self.kernel, self._sets = "", ()

    def _run(self, s_eq, t_eq, s_rows, t_rows, m):
        """dense (s_rows is None) or gathered (s_eq = t_eq = the full maps)"""
        out = torch.empty((m,), dtype=torch.float32, device=s_eq.device)
        fn = "buf_cost_volume_net" + self.kernel + ("" if s_rows is None else "_gather")
        head = (_ptr(s_eq), _ptr(t_eq), m) if s_rows is None else (_ptr(s_eq), 7, _ptr(s_rows), _ptr(t_rows), m)
        check(getattr(_lib.lib(), fn)(*head, self._wp, self._bp, *self._sets, _ptr(out), _stream()), fn)
        return out

    def __call__(self, s_eq, t_eq):
        """s_eq, t_eq f32[M,32,5,20] -> f32[M]"""
        s_eq, t_eq = s_eq.contiguous(), t_eq.contiguous()
        return self._run(s_eq, t_eq, None, None, s_eq.shape[0])

    def gathered(self, equi, s_rows, t_rows):
        """equi f32[rows,32,7,20] (full maps of all keypoints), s_rows / t_rows int64[M] -> f32[M]: the row gather and the
        elevation slice 1..5 (BUFFER.py:291-292) happen inside the kernel."""
        equi = _dev(equi, torch.float32, "CostVolumeNet.gathered")
        if equi.dim() != 4 or tuple(equi.shape[1:]) != (32, 7, 20):
            raise _lib.BufferHipError(f"CostVolumeNet.gathered: expected [rows,32,7,20] maps, got {tuple(equi.shape)}")
        s_rows, t_rows = _dev(s_rows, torch.int64, "s_rows"), _dev(t_rows, torch.int64, "t_rows")
        return self._run(equi, equi, s_rows, t_rows, int(s_rows.shape[0]))


class CostVolumeNetSplit:
    """CostNet on the f16 matrix pipe with fp32-equivalent arithmetic (csrc/costnet_h3.hip): opt-in next to CostVolumeNet, same calls.
    Layer 0 in its separated form (separate_cost_layer0), layer 1 with its three k' planes as channels, every layer direct form."""

    def __init__(self, layers, device, f24=None, f24b=None):
        """layers: 10 x (w [Cout,Cin,KD,KH,KW] np.float32 with BN folded, b [Cout]); f24, f24b: the fp32 re-run's layer forms, as in CostVolumeNet"""
        assert len(layers) == 10
        self.parts = cost_f24_parts(f24)
        self.parts_b = cost_f24b_parts(f24, f24b)
        mats = []
        w0 = layers[0][0]
        assert tuple(w0.shape) == (32, 32, 3, 3, 3), w0.shape
        ws, wt = separate_cost_layer0(w0)
        mats.append((np.transpose(ws.reshape(15, 32, 32), (2, 1, 0)), 2))                      # [o][c][dk*5 + e+2]
        mats.append((np.transpose(wt.reshape(9, 32, 32), (2, 1, 0)), 2))                       # [o][c][dk*3 + dl]
        w1 = layers[1][0]
        assert tuple(w1.shape) == (64, 32, 3, 3, 3), w1.shape
        mats.append((np.transpose(w1, (0, 3, 1, 2, 4)).reshape(64, 96, 9), 2))                 # [o][dk*32 + c][dn*3 + dl]
        for i in range(2, 9):
            w = layers[i][0]
            assert tuple(w.shape[2:]) == (3, 1, 3), w.shape
            mats.append((np.ascontiguousarray(w[:, :, :, 0, :]).reshape(w.shape[0], w.shape[1], 9), 2 if i < 7 else 1))
        w9 = layers[9][0]
        assert tuple(w9.shape) == (20, 32, 2, 1, 2), w9.shape
        mats.append((np.ascontiguousarray(w9[:, :, :, 0, :]).reshape(20, 32, 4), 1))
        self.wt = [torch.from_numpy(split_tile_gemm(m, nt).view(np.int16)).to(device) for m, nt in mats]
        self.bias = []
        for i, (_, b) in enumerate(layers):
            b = np.asarray(b, np.float32)
            if i == 9:
                b = np.concatenate([b, np.zeros(32 - b.shape[0], np.float32)])
            self.bias.append(torch.from_numpy(np.ascontiguousarray(b)).to(device))
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._wp = (C.c_void_p * 11)(*[t.data_ptr() for t in self.wt])
        self._bp = (C.c_void_p * 10)(*[t.data_ptr() for t in self.bias])
        # safe by construction (csrc/split_safe.hip): the fp32 kernel's weights ride along and re-run the matches the split kernel flags
        self.safe = not os.environ.get('BUF_SPLIT_UNSAFE')
        self.f32 = CostVolumeNet(layers, device, f24=f24, f24b=f24b) if self.safe else None
        self.last_flags = None

    def _safe(self, s_eq, t_eq, s_rows, t_rows, m, dev):
        out = torch.empty((m,), dtype=torch.float32, device=dev)
        self.last_flags = torch.empty((max(m, 1),), dtype=torch.int32, device=dev)
        fn = "buf_cost_volume_net_split_safe" + self.f32.kernel
        check(getattr(_lib.lib(), fn)(_ptr(s_eq), _ptr(t_eq), 7, _ptr(s_rows), _ptr(t_rows), m, self._wp, self._bp, self.f32._wp, self.f32._bp,
                                      *self.f32._sets, _ptr(out), _ptr(self.status), _ptr(self.last_flags), _stream()), fn)
        return out

    def __call__(self, s_eq, t_eq):
        """s_eq, t_eq f32[M,32,5,20] -> f32[M]"""
        L = _lib.lib()
        s_eq, t_eq = s_eq.contiguous(), t_eq.contiguous()
        m = s_eq.shape[0]
        if self.safe:
            return self._safe(s_eq, t_eq, None, None, m, s_eq.device)
        out = torch.empty((m,), dtype=torch.float32, device=s_eq.device)
        check(L.buf_cost_volume_net_split(_ptr(s_eq), _ptr(t_eq), m, self._wp, self._bp, _ptr(out), _ptr(self.status), _stream()),
              "buf_cost_volume_net_split")
        return out

    def gathered(self, equi, s_rows, t_rows):
        L = _lib.lib()
        equi = _dev(equi, torch.float32, "CostVolumeNetSplit.gathered")
        if equi.dim() != 4 or tuple(equi.shape[1:]) != (32, 7, 20):
            raise _lib.BufferHipError(f"CostVolumeNetSplit.gathered: expected [rows,32,7,20] maps, got {tuple(equi.shape)}")
        s_rows, t_rows = _dev(s_rows, torch.int64, "s_rows"), _dev(t_rows, torch.int64, "t_rows")
        m = int(s_rows.shape[0])
        if self.safe:
            return self._safe(equi, equi, s_rows, t_rows, m, equi.device)
        out = torch.empty((m,), dtype=torch.float32, device=equi.device)
        check(L.buf_cost_volume_net_split_gather(_ptr(equi), 7, _ptr(s_rows), _ptr(t_rows), m, self._wp, self._bp, _ptr(out),
                                                 _ptr(self.status), _stream()), "buf_cost_volume_net_split_gather")
        return out

    def range_fallbacks(self):
        """matches of the last call that left the f16 range and were recomputed by the fp32 kernel (synchronises)"""
        return 0 if self.last_flags is None else int((self.last_flags != 0).sum().item())

    def check_range(self):
        """Safe form: nothing to raise (flagged matches were recomputed in fp32); clears the informational status word."""
        if int(self.status.item()) != 0:
            self.status.zero_()
            if not self.safe:
                raise FloatingPointError("buf_cost_volume_net_split: a value left the f16 range (|v| >= 65504); use the fp32 kernel")
