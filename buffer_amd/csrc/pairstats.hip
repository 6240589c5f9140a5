// N4  Pair statistics under a GIVEN transform, for P pairs over C shared clouds per call: matches inside a distance, their
// squared residuals and the first and second moments of the matched target points (what overlap ratio, inlier RMSE and the
// 6x6 information matrix of a pair are made of).  The evaluation half of an ICP round (k_icp_correspond) without the loop.
//
//   buf_grid_build     ONE A2 cell grid over all C clouds, one element per cloud, radius = the correspondence distance; pair k
//                      searches element b_k.  A cloud is binned once however many pairs name it, as source or target.
//   k_pair_correspond  one workgroup per tile of PS_TILE source rows of one pair (tile -> pair through the tile prefix offsets).
//                      Per row the arithmetic of k_icp_correspond (a second copy of its candidate loop, kept apart so that the
//                      ICP kernels compile to what they were): p = T s in fp64, rounded to fp32 for the search, minimum 64-bit
//                      key (fp32 d2 bits, row) over the 9 x-runs with strict d2 < r2, non-finite rows skipped.  A hit adds, in
//                      fp64: 1, |p - u|^2 (unrounded p), u (3) and the upper triangle of u u^T (6), u in the target cloud's own
//                      frame.  Summed inside the wave and across the 4 waves in a fixed order; the tile writes ONE record.
//   k_pair_reduce      one wave per pair: the pair's records summed in a fixed order.
// No float atomics: a pair's 11 numbers are the same bits alone, in any batch, in any pair order, and across runs.
#include "common.h"

#define PS_TILE ICP_TILE
#define PS_NV 11
#define PS_STRIDE 12

__global__ void __launch_bounds__(PS_TILE) k_pair_correspond(const CellGrid* __restrict__ grids, const int* __restrict__ table,
                                                           const float4* __restrict__ sorted, const float* __restrict__ pts,
                                                           const int* __restrict__ cloud_off, const int* __restrict__ pair_a,
                                                           const int* __restrict__ pair_b, const int* __restrict__ tile_off,
                                                           const int* __restrict__ nn_off, int npairs, float r2,
                                                           const double* __restrict__ T, int* __restrict__ nn_out,
                                                           double* __restrict__ slab)
{
    __shared__ double part[ICP_WAVES][PS_NV];
    const int tile = blockIdx.x;
    const int k = find_elem(tile_off, npairs, tile);                       // uniform: a tile holds rows of one pair
    const int a = pair_a[k], b = pair_b[k];
    const int lo = cloud_off[a], n = cloud_off[a + 1] - lo, tlo = cloud_off[b];
    const int li = (tile - tile_off[k]) * PS_TILE + threadIdx.x;
    double v[PS_NV];
#pragma unroll
    for (int c = 0; c < PS_NV; c++) v[c] = 0.0;
    if (li < n) {
        const size_t i = (size_t)(lo + li);
        const double* Tb = T + 16 * (size_t)k;
        const double sx = pts[3 * i], sy = pts[3 * i + 1], sz = pts[3 * i + 2];
        const double px = ((Tb[0] * sx + Tb[1] * sy) + Tb[2] * sz) + Tb[3];
        const double py = ((Tb[4] * sx + Tb[5] * sy) + Tb[6] * sz) + Tb[7];
        const double pz = ((Tb[8] * sx + Tb[9] * sy) + Tb[10] * sz) + Tb[11];
        const float qx = (float)px, qy = (float)py, qz = (float)pz;      // the search runs on the fp32-rounded point
        int best = -1;
        if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
            const CellGrid g = grids[b];
            const int cx = query_cell_coord(qx, g.mn[0], g.inv_cell, g.dim[0]);
            const int cy = query_cell_coord(qy, g.mn[1], g.inv_cell, g.dim[1]);
            const int cz = query_cell_coord(qz, g.mn[2], g.inv_cell, g.dim[2]);
            unsigned long long key = ~0ull;
#pragma unroll 1                                                           // (one copy of the candidate loop)
            for (int j = 0; j < 9; j++) {
                int rs, len;
                cell_xrun(table, g.table_off, g.dim[0], g.dim[1], g.dim[2], cx, cy, cz, j, rs, len);
                for (int p = rs; p < rs + len; p++) {
                    const float4 c = sorted[p];
                    const float d2 = sqdist3(qx, qy, qz, c.x, c.y, c.z);
                    if (d2 < r2) {
                        const unsigned long long kk = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned int)__float_as_int(c.w);
                        key = kk < key ? kk : key;
                    }
                }
            }
            if (key != ~0ull) best = (int)(unsigned int)(key & 0xffffffffu) - tlo;      // row inside cloud b
        }
        if (nn_out) nn_out[(size_t)nn_off[k] + li] = best;
        if (best >= 0) {
            const size_t u = 3 * ((size_t)tlo + best);
            const double ux = pts[u], uy = pts[u + 1], uz = pts[u + 2];
            const double dx = px - ux, dy = py - uy, dz = pz - uz;
            v[0] = 1.0;
            v[1] = (dx * dx + dy * dy) + dz * dz;
            v[2] = ux; v[3] = uy; v[4] = uz;
            v[5] = ux * ux; v[6] = ux * uy; v[7] = ux * uz;
            v[8] = uy * uy; v[9] = uy * uz; v[10] = uz * uz;
        }
    }
    tile_sum<PS_NV, ICP_WAVES>(v, part, slab + (size_t)tile * PS_STRIDE);
}

__global__ void __launch_bounds__(WAVE) k_pair_reduce(const int* __restrict__ tile_off, const double* __restrict__ slab,
                                                    int* __restrict__ matched, double* __restrict__ moments)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const int t0 = tile_off[k], t1 = tile_off[k + 1];
    double v[PS_NV];
#pragma unroll
    for (int c = 0; c < PS_NV; c++) v[c] = 0.0;
    for (int t = t0 + lane; t < t1; t += WAVE) {
        const double* rec = slab + (size_t)t * PS_STRIDE;
#pragma unroll
        for (int c = 0; c < PS_NV; c++) v[c] += rec[c];
    }
#pragma unroll
    for (int c = 0; c < PS_NV; c++)
        for (int d = WAVE / 2; d > 0; d >>= 1) v[c] += __shfl_xor(v[c], d, WAVE);
    if (lane != 0) return;
    matched[k] = (int)v[0];
#pragma unroll
    for (int c = 1; c < PS_NV; c++) moments[10 * (size_t)k + c - 1] = v[c];
}

// ------------------------------------------------------------------------------------------
// n host ints -> device, by value in the kernel-argument block (the transport of upload_offsets, 896 ints = 3.5 KB per launch:
// the four index arrays of a 3540-pair call travel in 16 launches)
#define PS_INTS_PER_LAUNCH 896
struct IntChunk { int v[PS_INTS_PER_LAUNCH]; };

__global__ void __launch_bounds__(PS_INTS_PER_LAUNCH) k_store_ints(IntChunk c, int count, int* __restrict__ dst)
{
    if ((int)threadIdx.x < count) dst[threadIdx.x] = c.v[threadIdx.x];
}

static int upload_ints(int* dev, const int* host, long long n, const char* what, hipStream_t s)
{
    for (long long i0 = 0; i0 < n; i0 += PS_INTS_PER_LAUNCH) {
        IntChunk c;
        const int cnt = n - i0 < PS_INTS_PER_LAUNCH ? (int)(n - i0) : PS_INTS_PER_LAUNCH;
        for (int j = 0; j < cnt; j++) c.v[j] = host[i0 + j];
        k_store_ints<<<1, PS_INTS_PER_LAUNCH, 0, s>>>(c, cnt, dev + i0);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { buf_set_error("%s: upload -> %s", what, hipGetErrorString(e)); return BUF_EHIP; }
    return BUF_OK;
}

// the four index arrays of a call sit in ONE int region [pair_a (P) | pair_b (P) | tile_off (P + 1) | nn_off (P + 1)] and go up together
struct PairWs { void* grid; size_t grid_bytes; int* meta; int* pair_a; int* pair_b; int* tile_off; int* nn_off; double* slab; };

static PairWs carve_pairs(WsCarver& w, int n, int nclouds, int npairs, int n_src_rows, int64_t cells)
{
    PairWs e;
    e.grid_bytes = buf_grid_ws_bytes(n, nclouds, cells);
    e.grid = w.take<char>(e.grid_bytes);
    e.meta = w.take<int>(4 * (size_t)npairs + 2);
    e.pair_a = e.meta;
    e.pair_b = e.meta ? e.meta + npairs : nullptr;
    e.tile_off = e.meta ? e.meta + 2 * (size_t)npairs : nullptr;
    e.nn_off = e.meta ? e.meta + 3 * (size_t)npairs + 1 : nullptr;
    e.slab = w.take<double>((size_t)icp_tiles_upper(n_src_rows, npairs) * PS_STRIDE);
    return e;
}

extern "C" size_t buf_pair_stats_ws_bytes(int n_total, int nclouds, int npairs, int n_src_rows, int64_t cells_per_elem)
{
    if (n_total < 0 || nclouds <= 0 || npairs <= 0 || n_src_rows < 0) return 0;
    WsCarver w(nullptr, 0);
    carve_pairs(w, n_total, nclouds, npairs, n_src_rows, cells_per_elem);
    return w.used();
}

extern "C" int buf_pair_stats(const float* pts, const int* lengths_host, int nclouds, const int* pair_src_host,
                              const int* pair_tgt_host, int npairs, const double* T, float radius, int64_t cells_per_elem,
                              int* matched_out, double* moments_out, int* nn_out, void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(npairs >= 0 && nclouds >= 0, BUF_EINVAL, "buf_pair_stats: npairs=%d nclouds=%d", npairs, nclouds);
    BUF_REQUIRE(radius > 0.f && radius <= 3.4e38f, BUF_EINVAL, "buf_pair_stats: radius=%g (must be finite and > 0)", (double)radius);
    BUF_REQUIRE(nclouds == 0 || lengths_host, BUF_EINVAL, "buf_pair_stats: null lengths");
    long long n = 0;
    for (int c = 0; c < nclouds; c++) {
        BUF_REQUIRE(lengths_host[c] >= 0, BUF_EINVAL, "buf_pair_stats: negative length of cloud %d", c);
        n += lengths_host[c];
    }
    BUF_REQUIRE(n < 0x7fffffffLL, BUF_EINVAL, "buf_pair_stats: %lld points (int32 indices)", n);
    if (npairs == 0) return BUF_OK;
    BUF_REQUIRE(pair_src_host && pair_tgt_host, BUF_EINVAL, "buf_pair_stats: null pair list");
    BUF_REQUIRE(matched_out && moments_out, BUF_EINVAL, "buf_pair_stats: null output");
    BUF_REQUIRE(T && ws, BUF_EINVAL, "buf_pair_stats: null argument");
    BUF_REQUIRE(n == 0 || pts, BUF_EINVAL, "buf_pair_stats: null points");
    long long rows = 0, nts = 0;
    for (int k = 0; k < npairs; k++) {
        BUF_REQUIRE(pair_src_host[k] >= 0 && pair_src_host[k] < nclouds && pair_tgt_host[k] >= 0 && pair_tgt_host[k] < nclouds,
                    BUF_EINVAL, "buf_pair_stats: pair %d names clouds (%d, %d), outside [0, %d)", k, pair_src_host[k], pair_tgt_host[k],
                    nclouds);
        rows += lengths_host[pair_src_host[k]];
        nts += cdiv(lengths_host[pair_src_host[k]], PS_TILE);
    }
    BUF_REQUIRE(rows < 0x7fffffffLL, BUF_EINVAL, "buf_pair_stats: %lld source rows over all pairs (int32 indices)", rows);
    const size_t need = buf_pair_stats_ws_bytes((int)n, nclouds, npairs, (int)rows, cells_per_elem);
    BUF_REQUIRE(ws_bytes >= need, BUF_EWORKSPACE, "buf_pair_stats: workspace %zu < %zu bytes", ws_bytes, need);

    WsCarver w(ws, ws_bytes);
    const PairWs e = carve_pairs(w, (int)n, nclouds, npairs, (int)rows, cells_per_elem);
    buf_grid_t g;
    int rc = buf_grid_build(&g, pts, (int)n, lengths_host, nclouds, radius, cells_per_elem, e.grid, e.grid_bytes, s);
    if (rc) return rc;
    const size_t P = (size_t)npairs;
    int* meta = (int*)malloc(sizeof(int) * (4 * P + 2));
    BUF_REQUIRE(meta, BUF_EINVAL, "buf_pair_stats: out of host memory");
    int* tile_off = meta + 2 * P, *nn_off = meta + 3 * P + 1;
    tile_off[0] = 0; nn_off[0] = 0;
    for (size_t k = 0; k < P; k++) {
        const int len = lengths_host[pair_src_host[k]];
        meta[k] = pair_src_host[k];
        meta[P + k] = pair_tgt_host[k];
        tile_off[k + 1] = tile_off[k] + cdiv(len, PS_TILE);          // (totals checked above: < 2^31)
        nn_off[k + 1] = nn_off[k] + len;
    }
    rc = upload_ints(e.meta, meta, (long long)(4 * P + 2), "buf_pair_stats", s);
    free(meta);
    if (rc) return rc;
    const float r2 = radius * radius;                     // buf_grid_query's threshold
    if (nts > 0)
        k_pair_correspond<<<(int)nts, PS_TILE, 0, s>>>((const CellGrid*)g.desc, g.table, (const float4*)g.sorted, pts, g.s_off, e.pair_a,
                                                      e.pair_b, e.tile_off, e.nn_off, npairs, r2, T, nn_out, e.slab);
    k_pair_reduce<<<npairs, WAVE, 0, s>>>(e.tile_off, e.slab, matched_out, moments_out);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
