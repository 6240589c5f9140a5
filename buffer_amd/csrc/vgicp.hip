// N9 -- voxelized Generalized ICP (Koide, Yokozuka, Oishi, Banno, "Voxelized GICP for fast and accurate 3D point cloud registration",
// ICRA 2021; restated from the paper, no source at hand: parity unpinned) for B pairs per call against a REUSABLE map of target voxels.
// include/buffer_hip.h (N9) is the specification.
//
// Map (buf_voxel_map_build, once per set of target clouds; one readback of two ints at the end):
//   k_vg_bbox      one workgroup per cloud: the box of its points' voxel coordinates k = floor(p / voxel) (absolute origin), points
//                  with a non-finite coordinate or |k| >= 2^20 left out
//   k_vg_offsets   the clouds' dense tables laid one after the other (one slot per voxel of the box, x fastest, z slowest: ascending
//                  slot = ascending key); more than max_cells slots -> BUF_ECAPACITY
//   k_vg_count, scan, k_vg_scatter, k_vg_rank
//                  counting sort of the points by slot, every point ranked by input index inside its slot: a voxel's points are a
//                  contiguous run in INPUT order (the stable sort of subsample.hip / preprocess.hip restated on a table that is kept)
//   k_vg_emit      one lane per run head sums the run in input order: count, mean, mean of C(n) -> one row of ten doubles
//   k_vg_finish    table slot -> row of its voxel, -1 where the voxel is empty: the SAME table that sorted the points answers the
//                  lookups of every later registration call, one load per probed voxel
// Rounds (buf_vgicp_batched, two launches each, no host wait between rounds; the structure of icp.hip):
//   k_vg_terms<K>  one workgroup per tile of VG_TILE source points of one pair.  Per point: p = T s, its voxel, the K table slots of
//                  the neighbourhood loaded together (independent loads), the occupied ones kept in offset order in an LDS column,
//                  one term per occupied voxel; xor butterfly inside the wave, fixed sum over the 4 waves: ONE record per tile
//   k_vg_update    one wave per pair: records summed in a fixed order, fitness / rmse, N2's stopping rules, the 6x6 solve, T <- dT T
// All fp64 without FMA, every sum in a fixed order, no float atomics: a pair's result has the same bits alone, in any batch and on
// reruns.  The fp64 routines are those of pose_math.h; the update kernel body, the round loop and the tile offsets are icp.hip's.
#include "common.h"
#include "pose_math.h"
#include <limits.h>
#include <math.h>

#define VG_TILE 256
#define VG_WAVES (VG_TILE / WAVE)
#define VG_NV 30               // record: [0] terms, [1] points with a term, [2] sum |d|^2, [3..23] upper triangle of H, [24..29] g
#define VG_ROW 10              // map row: mean (3), covariance 00 01 02 11 12 22 (6), count
#define VG_KLIM 1048576.0      // 2^20

struct VgCloud { int mn[3]; int dim[3]; long long table_off; };     // dim = 0: no voxel
struct VgStatus { int error; int nrows; };
struct VgState { double prev_fit, prev_rmse; int done; int pad; };
struct VgRec {                                                       // (the record as pose_update of icp.hip reads it)
    static constexpr int NV = VG_NV, STRIDE = VG_NV, CNT = 0, FIT = 1, D2 = 2, H = 3, G = 24, MIN_CNT = 6;
    static constexpr bool KABSCH = false;
};

// voxel coordinates of a point; false for a point the map leaves out
__device__ __forceinline__ bool vg_voxel_of(double x, double y, double z, double voxel, int (&k)[3])
{
    const double kx = floor(x / voxel), ky = floor(y / voxel), kz = floor(z / voxel);
    if (!(fabs(kx) < VG_KLIM) || !(fabs(ky) < VG_KLIM) || !(fabs(kz) < VG_KLIM)) return false;     // (NaN and inf fail the comparison)
    k[0] = (int)kx; k[1] = (int)ky; k[2] = (int)kz;
    return true;
}

// ------------------------------------------------------------------------------------------ map build
__global__ void __launch_bounds__(256) k_vg_bbox(const float* __restrict__ pts, const int* __restrict__ off, double voxel,
                                               VgCloud* __restrict__ clouds)
{
    __shared__ int smn[3][4], smx[3][4];
    const int b = blockIdx.x, lo = off[b], hi = off[b + 1];
    int mn[3] = { INT_MAX, INT_MAX, INT_MAX }, mx[3] = { INT_MIN, INT_MIN, INT_MIN };
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        int k[3];
        if (!vg_voxel_of(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], voxel, k)) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) { mn[c] = min(mn[c], k[c]); mx[c] = max(mx[c], k[c]); }
    }
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int a = mn[c], z = mx[c];
        for (int d = WAVE / 2; d > 0; d >>= 1) { a = min(a, __shfl_xor(a, d, WAVE)); z = max(z, __shfl_xor(z, d, WAVE)); }
        if (lane == 0) { smn[c][w] = a; smx[c][w] = z; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        VgCloud g;
        for (int c = 0; c < 3; c++) {
            const int a = min(min(smn[c][0], smn[c][1]), min(smn[c][2], smn[c][3]));
            const int z = max(max(smx[c][0], smx[c][1]), max(smx[c][2], smx[c][3]));
            g.mn[c] = z >= a ? a : 0;
            g.dim[c] = z >= a ? z - a + 1 : 0;
        }
        g.table_off = 0;
        clouds[b] = g;
    }
}

__global__ void k_vg_offsets(VgCloud* __restrict__ clouds, int nclouds, long long max_cells, VgStatus* __restrict__ st)
{
    double run = 0.0;                                              // (a box has up to 2^63 voxels: counted in fp64, exact below 2^53)
    for (int b = 0; b < nclouds; b++) {
        clouds[b].table_off = run <= (double)max_cells ? (long long)run : 0;
        run += (double)clouds[b].dim[0] * (double)clouds[b].dim[1] * (double)clouds[b].dim[2];
    }
    st->error = run > (double)max_cells ? 1 : 0;
    st->nrows = 0;
}

// cnt[slot] += 1, flag[slot] = 1, slot_of[i] = the point's table slot (-1: left out)
__global__ void __launch_bounds__(256) k_vg_count(const float* __restrict__ pts, int n, const int* __restrict__ off, int nclouds,
                                                double voxel, const VgCloud* __restrict__ clouds, const VgStatus* __restrict__ st,
                                                int* __restrict__ cnt, int* __restrict__ flag, int* __restrict__ slot_of)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || st->error) return;
    const int b = nclouds > 1 ? find_elem(off, nclouds, i) : 0;
    const VgCloud g = clouds[b];
    int k[3], slot = -1;
    if (vg_voxel_of(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], voxel, k))
        slot = (int)(g.table_off + (k[0] - g.mn[0]) + (long long)g.dim[0] * ((k[1] - g.mn[1]) + (long long)g.dim[1] * (k[2] - g.mn[2])));
    slot_of[i] = slot;
    if (slot >= 0) { atomicAdd(&cnt[slot], 1); flag[slot] = 1; }
}

// cnt holds exclusive slot starts on entry and inclusive slot ends after
__global__ void __launch_bounds__(256) k_vg_scatter(int n, const int* __restrict__ slot_of, const VgStatus* __restrict__ st,
                                                  int* __restrict__ cnt, int* __restrict__ sorted)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || st->error) return;
    const int slot = slot_of[i];
    if (slot >= 0) sorted[atomicAdd(&cnt[slot], 1)] = i;
}

// the scatter order inside a slot depends on atomic arrival: every point ranks itself by input index inside its run
__global__ void __launch_bounds__(256) k_vg_rank(int n, long long max_cells, const int* __restrict__ slot_of,
                                               const VgStatus* __restrict__ st, const int* __restrict__ cnt,
                                               const int* __restrict__ sorted_in, int* __restrict__ sorted_out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n || st->error || p >= cnt[max_cells]) return;          // cnt[max_cells] = points in the map
    const int i = sorted_in[p], slot = slot_of[i];
    const int s = slot == 0 ? 0 : cnt[slot - 1], e = cnt[slot];
    int rank = 0;
    for (int t = s; t < e; t++) rank += sorted_in[t] < i ? 1 : 0;
    sorted_out[s + rank] = i;
}

__global__ void __launch_bounds__(256) k_vg_emit(const float* __restrict__ pts, const float* __restrict__ normals, int n,
                                               long long max_cells, double voxel, double w, const int* __restrict__ slot_of,
                                               const VgStatus* __restrict__ st, const int* __restrict__ cnt,
                                               const int* __restrict__ sorted, const int* __restrict__ rowscan,
                                               double* __restrict__ rows, long long* __restrict__ keys)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n || st->error || p >= cnt[max_cells]) return;
    const int i0 = sorted[p], slot = slot_of[i0];
    if (p != (slot == 0 ? 0 : cnt[slot - 1])) return;               // not the head of its run
    const int e = cnt[slot];
    double sm[3] = { 0.0, 0.0, 0.0 }, sc[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int t = p; t < e; t++) {                                    // input order
        const size_t i = (size_t)sorted[t];
        double nn[3];
        unit_normal_or_zero(normals, i, nn);
        int k = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            sm[r] += (double)pts[3 * i + r];
#pragma unroll
            for (int c = r; c < 3; c++) sc[k++] += (r == c ? 1.0 : 0.0) - (w * nn[r]) * nn[c];      // C(n) = I - (1 - epsilon) n n^T
        }
    }
    const double N = (double)(e - p);
    double* row = rows + VG_ROW * (size_t)rowscan[slot];
#pragma unroll
    for (int r = 0; r < 3; r++) row[r] = sm[r] / N;
#pragma unroll
    for (int k = 0; k < 6; k++) row[3 + k] = sc[k] / N;
    row[9] = N;
    int kv[3];
    vg_voxel_of(pts[3 * (size_t)i0], pts[3 * (size_t)i0 + 1], pts[3 * (size_t)i0 + 2], voxel, kv);
    keys[rowscan[slot]] = ((long long)(kv[2] + 1048576) << 42) | ((long long)(kv[1] + 1048576) << 21) | (long long)(kv[0] + 1048576);
}

// row ranges of the clouds from the exclusive flag scan (rowscan[max_cells] = its total) and the status record
__global__ void k_vg_row_off(const VgCloud* __restrict__ clouds, int nclouds, long long max_cells, const int* __restrict__ rowscan,
                             VgStatus* __restrict__ st, int* __restrict__ row_off)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nclouds) return;
    const bool bad = st->error != 0;
    row_off[b] = bad ? 0 : (b < nclouds ? rowscan[clouds[b].table_off] : rowscan[max_cells]);
    if (b == nclouds) st->nrows = bad ? 0 : rowscan[max_cells];
}

// table slot: the row of its voxel, -1 where the voxel holds no point (in place on the exclusive flag scan)
__global__ void __launch_bounds__(256) k_vg_finish(long long max_cells, const VgStatus* __restrict__ st, const int* __restrict__ cnt,
                                                 int* __restrict__ table)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= max_cells) return;
    const bool occupied = !st->error && cnt[c] - (c == 0 ? 0 : cnt[c - 1]) > 0;
    if (!occupied) table[c] = -1;
}

__global__ void __launch_bounds__(256) k_vg_export(const double* __restrict__ rows, int nrows, int* __restrict__ counts,
                                                 double* __restrict__ means, double* __restrict__ covs)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    const double* row = rows + VG_ROW * (size_t)r;
    for (int c = 0; c < 3; c++) means[3 * (size_t)r + c] = row[c];
    for (int c = 0; c < 6; c++) covs[6 * (size_t)r + c] = row[3 + c];
    counts[r] = (int)row[9];
}

struct VgMapBuf { VgCloud* clouds; int* table; double* rows; long long* keys; int* row_off; };

static VgMapBuf carve_vg_map(WsCarver& w, int n, int nclouds, long long max_cells)
{
    VgMapBuf m;
    m.clouds = w.take<VgCloud>((size_t)nclouds);
    m.table = w.take<int>((size_t)max_cells + 1);
    m.rows = w.take<double>(VG_ROW * (size_t)n);
    m.keys = w.take<long long>((size_t)n);
    m.row_off = w.take<int>((size_t)nclouds + 1);
    return m;
}

struct VgBuildWs { int* off; int* cnt; int* slot_of; int* sorted_tmp; int* sorted; int* scan_tmp; VgStatus* st; };

static VgBuildWs carve_vg_build(WsCarver& w, int n, int nclouds, long long max_cells)
{
    VgBuildWs v;
    v.off = w.take<int>((size_t)nclouds + 1);
    v.cnt = w.take<int>((size_t)max_cells + 1);
    v.slot_of = w.take<int>((size_t)n);
    v.sorted_tmp = w.take<int>((size_t)n);
    v.sorted = w.take<int>((size_t)n);
    v.scan_tmp = w.take<int>(scan_tmp_ints());
    v.st = w.take<VgStatus>(1);
    return v;
}

static bool vg_sizes_ok(int n, int nclouds, long long max_cells) { return n >= 0 && nclouds > 0 && nclouds <= 65535 && max_cells >= 1 && max_cells < 0x7fffffffLL; }

extern "C" size_t buf_voxel_map_bytes(int n_total, int nclouds, int64_t max_cells)
{
    if (!vg_sizes_ok(n_total, nclouds, max_cells)) return 0;
    WsCarver w(nullptr, 0);
    carve_vg_map(w, n_total, nclouds, max_cells);
    return w.used();
}

extern "C" size_t buf_voxel_map_ws_bytes(int n_total, int nclouds, int64_t max_cells)
{
    if (!vg_sizes_ok(n_total, nclouds, max_cells)) return 0;
    WsCarver w(nullptr, 0);
    carve_vg_build(w, n_total, nclouds, max_cells);
    return w.used();
}

extern "C" int buf_voxel_map_build(buf_voxel_map_t* map, const float* pts, const float* normals, const int* lengths_host, int nclouds,
                                   double voxel, double epsilon, int64_t max_cells, void* buf, size_t buf_bytes, void* ws,
                                   size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(map && lengths_host, BUF_EINVAL, "buf_voxel_map_build: null argument");
    BUF_REQUIRE(voxel > 0.0 && voxel <= 1.7e308, BUF_EINVAL, "buf_voxel_map_build: voxel=%g (must be finite and > 0)", voxel);
    BUF_REQUIRE(epsilon > 0.0 && epsilon <= 1.0, BUF_EINVAL, "buf_voxel_map_build: epsilon=%g (must be in (0, 1])", epsilon);
    BUF_REQUIRE(nclouds > 0 && nclouds <= 65535, BUF_EINVAL, "buf_voxel_map_build: nclouds=%d (1..65535)", nclouds);
    long long nl = 0;
    for (int b = 0; b < nclouds; b++) {
        BUF_REQUIRE(lengths_host[b] >= 0, BUF_EINVAL, "buf_voxel_map_build: negative length in cloud %d", b);
        nl += lengths_host[b];
    }
    BUF_REQUIRE(nl < 0x7fffffffLL, BUF_EINVAL, "buf_voxel_map_build: %lld points (int32 indices)", nl);
    BUF_REQUIRE(max_cells >= 1 && max_cells < 0x7fffffffLL, BUF_EINVAL, "buf_voxel_map_build: max_cells=%lld", (long long)max_cells);
    const int n = (int)nl;
    BUF_REQUIRE(n == 0 || pts, BUF_EINVAL, "buf_voxel_map_build: null points");
    BUF_REQUIRE(buf && ws, BUF_EINVAL, "buf_voxel_map_build: null buffer");
    BUF_REQUIRE(buf_bytes >= buf_voxel_map_bytes(n, nclouds, max_cells), BUF_EWORKSPACE, "buf_voxel_map_build: map buffer %zu < %zu bytes",
                buf_bytes, buf_voxel_map_bytes(n, nclouds, max_cells));
    BUF_REQUIRE(ws_bytes >= buf_voxel_map_ws_bytes(n, nclouds, max_cells), BUF_EWORKSPACE, "buf_voxel_map_build: workspace %zu < %zu bytes",
                ws_bytes, buf_voxel_map_ws_bytes(n, nclouds, max_cells));
    WsCarver wm(buf, buf_bytes), ww(ws, ws_bytes);
    const VgMapBuf m = carve_vg_map(wm, n, nclouds, max_cells);
    const VgBuildWs v = carve_vg_build(ww, n, nclouds, max_cells);
    memset(map, 0, sizeof(*map));

    int rc = upload_offsets(v.off, lengths_host, nclouds, n, "buf_voxel_map_build", s);
    if (rc) return rc;
    const size_t tbytes = sizeof(int) * ((size_t)max_cells + 1);
    BUF_CHECK_HIP(hipMemsetAsync(v.cnt, 0, tbytes, s));
    BUF_CHECK_HIP(hipMemsetAsync(m.table, 0, tbytes, s));
    k_vg_bbox<<<nclouds, 256, 0, s>>>(pts, v.off, voxel, m.clouds);
    k_vg_offsets<<<1, 1, 0, s>>>(m.clouds, nclouds, (long long)max_cells, v.st);
    const int blocks = cdiv(n, 256);
    if (n > 0) k_vg_count<<<blocks, 256, 0, s>>>(pts, n, v.off, nclouds, voxel, m.clouds, v.st, v.cnt, m.table, v.slot_of);
    rc = exclusive_scan_i32(v.cnt, (long long)max_cells + 1, v.scan_tmp, nullptr, s);
    if (rc) return rc;
    rc = exclusive_scan_i32(m.table, (long long)max_cells + 1, v.scan_tmp, nullptr, s);
    if (rc) return rc;
    if (n > 0) {
        k_vg_scatter<<<blocks, 256, 0, s>>>(n, v.slot_of, v.st, v.cnt, v.sorted_tmp);
        k_vg_rank<<<blocks, 256, 0, s>>>(n, (long long)max_cells, v.slot_of, v.st, v.cnt, v.sorted_tmp, v.sorted);
        k_vg_emit<<<blocks, 256, 0, s>>>(pts, normals, n, (long long)max_cells, voxel, 1.0 - epsilon, v.slot_of, v.st, v.cnt, v.sorted, m.table,
                                         m.rows, m.keys);
    }
    k_vg_row_off<<<cdiv(nclouds + 1, 64), 64, 0, s>>>(m.clouds, nclouds, (long long)max_cells, m.table, v.st, m.row_off);
    k_vg_finish<<<cdiv(max_cells, 256), 256, 0, s>>>((long long)max_cells, v.st, v.cnt, m.table);
    BUF_LAUNCH_CHECK();
    VgStatus hs;
    hipError_t e = hipMemcpyAsync(&hs, v.st, sizeof(hs), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    BUF_CHECK_HIP(e);
    BUF_REQUIRE(!hs.error, BUF_ECAPACITY, "buf_voxel_map_build: the clouds' voxel boxes do not fit max_cells=%lld", (long long)max_cells);
    map->buf = buf; map->buf_bytes = buf_bytes;
    map->nclouds = nclouds; map->nrows = hs.nrows; map->n = n;
    map->max_cells = max_cells;
    map->voxel = voxel; map->epsilon = epsilon;
    map->clouds = m.clouds; map->table = m.table; map->rows = m.rows; map->keys = m.keys; map->row_off = m.row_off;
    return BUF_OK;
}

extern "C" int buf_voxel_map_export(const buf_voxel_map_t* map, int n, long long* keys, int* counts, double* means, double* covs,
                                    int* row_off, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(map && map->buf && row_off, BUF_EINVAL, "buf_voxel_map_export: null argument");
    BUF_REQUIRE(n >= map->nrows, BUF_EINVAL, "buf_voxel_map_export: capacity %d < %d rows", n, map->nrows);
    BUF_CHECK_HIP(hipMemcpyAsync(row_off, map->row_off, sizeof(int) * ((size_t)map->nclouds + 1), hipMemcpyDeviceToDevice, s));
    if (map->nrows == 0) return BUF_OK;
    BUF_REQUIRE(keys && counts && means && covs, BUF_EINVAL, "buf_voxel_map_export: null output");
    BUF_CHECK_HIP(hipMemcpyAsync(keys, map->keys, sizeof(long long) * (size_t)map->nrows, hipMemcpyDeviceToDevice, s));
    k_vg_export<<<cdiv(map->nrows, 256), 256, 0, s>>>((const double*)map->rows, map->nrows, counts, means, covs);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}

// ------------------------------------------------------------------------------------------ registration
__global__ void __launch_bounds__(WAVE) k_vg_setup(int npairs, const double* __restrict__ T_init, double* __restrict__ T,
                                                 double* __restrict__ fitness, double* __restrict__ rmse, int* __restrict__ iters,
                                                 VgState* __restrict__ st)
{
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if (b >= npairs) return;
    for (int k = 0; k < 16; k++) T[16 * (size_t)b + k] = T_init[16 * (size_t)b + k];
    VgState s;
    s.prev_fit = 0.0; s.prev_rmse = 0.0; s.done = 0; s.pad = 0;
    st[b] = s;
    fitness[b] = 0.0; rmse[b] = 0.0; iters[b] = 0;
}

// offset j of a neighbourhood of K voxels.  1: the voxel; 7: the voxel, +x, -x, +y, -y, +z, -z; 27: dz outermost, dx innermost, -1 0 +1
template <int K> __device__ __forceinline__ constexpr int vg_off(int j, int axis)
{
    if (K == 27) return (axis == 0 ? j % 3 : axis == 1 ? (j / 3) % 3 : j / 9) - 1;
    if (K == 7) return j == 0 || (j - 1) / 2 != axis ? 0 : ((j - 1) % 2 == 0 ? 1 : -1);
    return 0;
}

template <int K>
__global__ void __launch_bounds__(VG_TILE) k_vg_terms(const VgCloud* __restrict__ clouds, const int* __restrict__ table,
                                                    const double* __restrict__ rows, const int* __restrict__ row_off,
                                                    const int* __restrict__ pair_cloud, const float* __restrict__ src,
                                                    const float* __restrict__ src_normals, const int* __restrict__ src_off,
                                                    const int* __restrict__ tile_off, int npairs, double voxel, double w,
                                                    const double* __restrict__ T, const VgState* __restrict__ st,
                                                    int* __restrict__ row_out, double* __restrict__ slab)
{
    __shared__ double part[VG_WAVES][VG_NV];
    __shared__ int hit[K][VG_TILE];                                    // a thread's occupied rows, in offset order (its own column)
    const int tile = blockIdx.x;
    const int b = find_elem(tile_off, npairs, tile);                   // uniform: a tile holds points of one pair
    if (st[b].done) return;
    const int lo = src_off[b], n = src_off[b + 1] - lo;
    const int li = (tile - tile_off[b]) * VG_TILE + threadIdx.x;
    double v[VG_NV];
#pragma unroll
    for (int k = 0; k < VG_NV; k++) v[k] = 0.0;
    if (li < n) {
        const size_t i = (size_t)(lo + li);
        const int pc = pair_cloud[b];
        const double* Tb = T + 16 * (size_t)b;
        const double sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
        const double p[3] = { ((Tb[0] * sx + Tb[1] * sy) + Tb[2] * sz) + Tb[3], ((Tb[4] * sx + Tb[5] * sy) + Tb[6] * sz) + Tb[7],
                              ((Tb[8] * sx + Tb[9] * sy) + Tb[10] * sz) + Tb[11] };
        int kq[3], nhit = 0, own = -1;
        // (|k| < 2^20 as on the build side: a point further out has no neighbour in any map; NaN and inf fail it too)
        if (vg_voxel_of(p[0], p[1], p[2], voxel, kq)) {
            const VgCloud g = clouds[pc];
            int r[K];
#pragma unroll
            for (int j = 0; j < K; j++) {                              // K independent loads, none waits for another
                const int x = kq[0] + vg_off<K>(j, 0) - g.mn[0], y = kq[1] + vg_off<K>(j, 1) - g.mn[1], z = kq[2] + vg_off<K>(j, 2) - g.mn[2];
                const bool in = x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2];
                const long long slot = in ? g.table_off + x + (long long)g.dim[0] * (y + (long long)g.dim[1] * z) : 0;
                const int t = table[slot];
                r[j] = in ? t : -1;
            }
            own = r[K / 2 == 13 ? 13 : 0];
#pragma unroll
            for (int j = 0; j < K; j++)
                if (r[j] >= 0) hit[nhit++][threadIdx.x] = r[j];
        }
        if (row_out) row_out[i] = own >= 0 ? own - row_off[pc] : -1;
        if (nhit > 0) {
            double ns[3], m[3], RR[6];
            unit_normal_or_zero(src_normals, i, ns);
#pragma unroll
            for (int r = 0; r < 3; r++) m[r] = (Tb[4 * r] * ns[0] + Tb[4 * r + 1] * ns[1]) + Tb[4 * r + 2] * ns[2];
            {
                int k = 0;
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = r; c < 3; c++) RR[k++] = (Tb[4 * r] * Tb[4 * c] + Tb[4 * r + 1] * Tb[4 * c + 1]) + Tb[4 * r + 2] * Tb[4 * c + 2];
            }
            v[1] = 1.0;
#pragma unroll 1                                                       // (one copy of the term)
            for (int j = 0; j < nhit; j++) {
                const double* row = rows + VG_ROW * (size_t)hit[j][threadIdx.x];
                const double Nv = row[9];
                const double dx = p[0] - row[0], dy = p[1] - row[1], dz = p[2] - row[2];
                // S = cov_v + R C(n_s) R^T = cov_v + (R R^T - w m m^T), m = R n_s; upper triangle 00 01 02 11 12 22
                double S[6];
                {
                    int k = 0;
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = r; c < 3; c++) { S[k] = (row[3 + k] + RR[k]) - (w * m[r]) * m[c]; k++; }
                }
                GicpTerm gt;
                gicp_term(S, p, dx, dy, dz, gt);
                v[0] += 1.0;
                v[2] += (dx * dx + dy * dy) + dz * dz;
                int k = 3;
#pragma unroll
                for (int r = 0; r < 3; r++) {                          // rows 0..2 of H: [A^T M A | A^T M], A^T M = (M A)^T
#pragma unroll
                    for (int c = r; c < 3; c++) v[k++] += Nv * gt.AtMA[r][c];
#pragma unroll
                    for (int c = 0; c < 3; c++) v[k++] += Nv * gt.MA[c][r];
                }
#pragma unroll
                for (int r = 0; r < 3; r++)                            // rows 3..5: M
#pragma unroll
                    for (int c = r; c < 3; c++) v[k++] += Nv * gt.Mm[r][c];
#pragma unroll
                for (int r = 0; r < 3; r++) { v[24 + r] += Nv * gt.AtMd[r]; v[27 + r] += Nv * gt.Md[r]; }
            }
        }
    }
    tile_sum<VG_NV, VG_WAVES>(v, part, slab + (size_t)tile * VG_NV);
}

__global__ void __launch_bounds__(WAVE) k_vg_update(const int* __restrict__ src_off, const int* __restrict__ tile_off,
                                                  const double* __restrict__ slab, int max_iteration, double rel_fitness,
                                                  double rel_rmse, double* __restrict__ T, double* __restrict__ fitness,
                                                  double* __restrict__ rmse_out, int* __restrict__ iters, VgState* __restrict__ st,
                                                  int* __restrict__ active)
{
    pose_update<VgRec>(src_off, tile_off, slab, max_iteration, rel_fitness, rel_rmse, T, fitness, rmse_out, iters, st, active);
}

struct VgWs { int* src_off; int* tile_off; int* pair_cloud; VgState* st; double* slab; int* active; };

static VgWs carve_vgicp(WsCarver& w, int ns, int npairs)
{
    VgWs e;
    e.src_off = w.take<int>((size_t)npairs + 1);
    e.tile_off = w.take<int>((size_t)npairs + 1);
    e.pair_cloud = w.take<int>((size_t)npairs);
    e.st = w.take<VgState>((size_t)npairs);
    e.slab = w.take<double>((size_t)(cdiv(ns, VG_TILE) + npairs) * VG_NV);
    e.active = w.take<int>(64);
    return e;
}

extern "C" size_t buf_vgicp_ws_bytes(int n_src_total, int npairs)
{
    if (n_src_total < 0 || npairs <= 0) return 0;
    WsCarver w(nullptr, 0);
    carve_vgicp(w, n_src_total, npairs);
    return w.used();
}

template <int K>
static int vg_rounds(const VgWs& e, const buf_voxel_map_t* map, const float* src, const float* src_normals, int npairs, int ntiles,
                     int max_iteration, double rel_fitness, double rel_rmse, double* T_out, double* fitness_out, double* rmse_out,
                     int* iters_out, int* row_out, hipStream_t s)
{
    const auto terms = [&] {
        if (ntiles > 0)
            k_vg_terms<K><<<ntiles, VG_TILE, 0, s>>>((const VgCloud*)map->clouds, map->table, map->rows, map->row_off, e.pair_cloud, src,
                                                     src_normals, e.src_off, e.tile_off, npairs, map->voxel, 1.0 - map->epsilon, T_out,
                                                     e.st, row_out, e.slab);
    };
    return pose_rounds(e, terms, k_vg_update, npairs, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out, iters_out, s);
}

extern "C" int buf_vgicp_batched(const buf_voxel_map_t* map, const float* src, const float* src_normals, const int* src_lengths_host,
                                 const int* pair_cloud_host, int npairs, int neighbors, const double* T_init, int max_iteration,
                                 double rel_fitness, double rel_rmse, double* T_out, double* fitness_out, double* rmse_out,
                                 int* iters_out, int* row_out, void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(map && map->buf && map->nclouds > 0, BUF_EINVAL, "buf_vgicp_batched: no voxel map");
    BUF_REQUIRE(npairs >= 0 && npairs <= 65535, BUF_EINVAL, "buf_vgicp_batched: npairs=%d (0..65535)", npairs);
    BUF_REQUIRE(neighbors == 1 || neighbors == 7 || neighbors == 27, BUF_EINVAL, "buf_vgicp_batched: neighbors=%d (1, 7 or 27)", neighbors);
    BUF_REQUIRE(max_iteration >= 0, BUF_EINVAL, "buf_vgicp_batched: max_iteration=%d", max_iteration);
    if (npairs == 0) return BUF_OK;
    BUF_REQUIRE(src_lengths_host, BUF_EINVAL, "buf_vgicp_batched: null lengths");
    BUF_REQUIRE(pair_cloud_host || npairs <= map->nclouds, BUF_EINVAL, "buf_vgicp_batched: %d pairs but %d map clouds and no pair_cloud",
                npairs, map->nclouds);
    long long ns = 0;
    for (int b = 0; b < npairs; b++) {
        BUF_REQUIRE(src_lengths_host[b] >= 0, BUF_EINVAL, "buf_vgicp_batched: negative length in pair %d", b);
        BUF_REQUIRE(!pair_cloud_host || (pair_cloud_host[b] >= 0 && pair_cloud_host[b] < map->nclouds), BUF_EINVAL,
                    "buf_vgicp_batched: pair_cloud[%d]=%d outside the map's %d clouds", b, pair_cloud_host ? pair_cloud_host[b] : 0, map->nclouds);
        ns += src_lengths_host[b];
    }
    BUF_REQUIRE(ns < 0x7fffffffLL, BUF_EINVAL, "buf_vgicp_batched: %lld points (int32 indices)", ns);
    BUF_REQUIRE(ns == 0 || src, BUF_EINVAL, "buf_vgicp_batched: null src");
    BUF_REQUIRE(T_init && T_out && fitness_out && rmse_out && iters_out && ws, BUF_EINVAL, "buf_vgicp_batched: null argument");
    const size_t need = buf_vgicp_ws_bytes((int)ns, npairs);
    BUF_REQUIRE(ws_bytes >= need, BUF_EWORKSPACE, "buf_vgicp_batched: workspace %zu < %zu bytes", ws_bytes, need);

    WsCarver w(ws, ws_bytes);
    const VgWs e = carve_vgicp(w, (int)ns, npairs);
    int rc = upload_offsets(e.src_off, src_lengths_host, npairs, (int)ns, "buf_vgicp_batched", s);
    if (rc) return rc;
    int nts = 0;
    rc = upload_tile_offsets(e.tile_off, src_lengths_host, npairs, VG_TILE, "buf_vgicp_batched", &nts, s);
    if (rc) return rc;
    for (int b0 = 0; b0 < npairs; b0 += OFFS_PER_LAUNCH) {               // the pairs' clouds, by value in the argument block
        OffsetChunk c;
        const int cntb = npairs - b0 < OFFS_PER_LAUNCH ? npairs - b0 : OFFS_PER_LAUNCH;
        for (int t = 0; t < OFFS_PER_LAUNCH; t++) c.v[t] = t < cntb ? (pair_cloud_host ? pair_cloud_host[b0 + t] : b0 + t) : 0;
        k_store_offsets<<<1, OFFS_PER_LAUNCH, 0, s>>>(c, cntb, e.pair_cloud + b0);
    }
    if (row_out && ns > 0) BUF_CHECK_HIP(hipMemsetAsync(row_out, 0xff, sizeof(int) * (size_t)ns, s));       // -1
    k_vg_setup<<<cdiv(npairs, WAVE), WAVE, 0, s>>>(npairs, T_init, T_out, fitness_out, rmse_out, iters_out, e.st);
    BUF_LAUNCH_CHECK();
    if (neighbors == 1)
        return vg_rounds<1>(e, map, src, src_normals, npairs, nts, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out,
                            iters_out, row_out, s);
    if (neighbors == 7)
        return vg_rounds<7>(e, map, src, src_normals, npairs, nts, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out,
                            iters_out, row_out, s);
    return vg_rounds<27>(e, map, src, src_normals, npairs, nts, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out,
                         iters_out, row_out, s);
}
