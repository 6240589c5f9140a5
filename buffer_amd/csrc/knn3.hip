// N14 -- exact k nearest neighbours in 3-D on the cell grid of radius.hip (open3d KDTreeSearchParamKNN), and
// N15 -- the per-cloud sums of open3d's remove_statistical_outlier on the rows N14 returns.
//
// k_grid_knn: one wavefront per query, a ring search on the dense table.
//   The query's cell c = query_cell_coord clamped into the grid.  Ring rho = the cells at Chebyshev distance rho from c, clipped to
//   the grid, visited as x-runs: a (y, z) row on the shell of the cube (max(|dy|, |dz|) == rho) is ONE run of cells
//   [cx - rho, cx + rho], an inner row contributes its two end cells.  The lanes fetch the run bounds of 64 rows at a time (two table
//   reads per run, as cell_xrun does); a ballot then walks the non-empty runs only, so an empty ring costs rows / 64 steps.
//   The k best keys (d2 bits << 32 | global index) live one per lane, ascending (lane i = rank i, ~0 = empty slot).  A chunk of 64
//   candidates is tested against the k-th key at once; the survivors are inserted one by one: broadcast (readlane), every lane
//   compares, the lanes above the insertion point take their lower neighbour's key.  No LDS, no atomics, no scratch.
//   After ring rho the search stops once the k-th d2 lies strictly below knn_ring_bound (the derivation stands there), or once the
//   cube covers the element's whole grid.  rho <= max(dim): the loop ends on any input; every trip condition is wave-uniform (the
//   query is).
// A pair whose fp32 d2 is not finite (a NaN / infinite coordinate on either side, or an overflow) matches nothing: buf_grid_query's
// d2 < r*r can never accept such a pair either.
#include "common.h"

#define KNN_WAVES 4
#define KNN_MAX_K 64
#define KNN_EMPTY (~0ull)

__device__ __forceinline__ unsigned long long wave_bcast_u64(unsigned long long v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// Squared distance (fp32) below which the k-th key closes the search after ring rho, 0 = go on.
//   f[a] = (double(q_a) - double(mn_a)) * inv_cell, the build's own arithmetic (cell_coord), c[a] = the query's clamped cell.
//   The cube is [c - rho, c + rho + 1) in cell units on every axis.  A face at an integer m that lies strictly inside the grid
//   (1 <= m <= dim - 1) separates the supports: the build puts a finite support into cell >= m iff its own computed f_s >= m (floor is
//   monotone and the clamps act at the grid's faces only).  Both f's carry two fp64 roundings (the subtraction, the product):
//   f = f_exact (1 + e), |e| < 2^-52, so in units of 1 / inv_cell the true coordinate gap to the face is at least
//   |m - f| - 2^-52 (|m| + |f|); the code subtracts 2^-50 (|m| + |f| + 1).  Dividing by inv_cell adds 2^-53 relative.
//   fp32 side: for a support beyond the face |fl(q - s)| >= gap (1 - 2^-24), its square and the two additions of non-negative terms
//   round three more times: sqdist3 >= gap^2 (1 - 2^-24)^5 > gap^2 (1 - 2^-21), as long as gap^2 is a normal fp32 number.  The bound
//   returned is (float)(gap^2 (1 - 2^-20)) -- the conversion rounds by at most 2^-24 relative, so bound < every sqdist3 beyond the
//   face -- and 0 when gap^2 < 2^-100 (far above the smallest normal 2^-126: products that underflow lose their relative bound).
//   "k-th d2 < bound" therefore puts every support outside the cube strictly above the k-th key, whatever its index.
//   The margin of a face may come out zero or negative -- a query whose f is an inner integer m exactly, or within 2^-50 (2 m + 1) of
//   one, sits ON the face of its own cell at rho = 0 -- and such a face says nothing about the supports beyond it: the minimum over the
//   faces keeps that value (fmin throughout, +inf = no face seen yet) and the bound is 0.
__device__ __forceinline__ float knn_ring_bound(const double f[3], const int c[3], const int dim[3], int rho, double inv_cell, bool& covers)
{
    double gap = __builtin_inf();                        // the smallest margin over the cube's faces inside the grid; it may be <= 0 (go on)
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int lo = c[a] - rho, hi = c[a] + rho + 1;          // faces of the cube on this axis (rho <= max dim < 2^31 / 2: no overflow)
        if (lo >= 1) {
            const double g = (f[a] - (double)lo) - 0x1p-50 * ((double)lo + fabs(f[a]) + 1.0);
            gap = fmin(gap, g);
        }
        if (hi <= dim[a] - 1) {
            const double g = ((double)hi - f[a]) - 0x1p-50 * ((double)hi + fabs(f[a]) + 1.0);
            gap = fmin(gap, g);
        }
    }
    // no face inside the grid <=> the cube covers the grid (lo >= 1 and hi <= dim - 1 above are the negations of these six)
    covers = c[0] - rho <= 0 && c[1] - rho <= 0 && c[2] - rho <= 0 && c[0] + rho >= dim[0] - 1 &&
             c[1] + rho >= dim[1] - 1 && c[2] + rho >= dim[2] - 1;
    if (covers || !(gap > 0.0)) return 0.f;              // a query on a face (within the margin) has gap <= 0 there: the next ring is visited
    const double gr = gap / inv_cell;
    const double g2 = gr * gr * (1.0 - 0x1p-20);
    return g2 >= 0x1p-100 ? (float)g2 : 0.f;
}

__global__ void __launch_bounds__(KNN_WAVES * WAVE) k_grid_knn(const CellGrid* __restrict__ grids, const int* __restrict__ table,
                                                             const float4* __restrict__ sorted, const float* __restrict__ queries, int nq,
                                                             const int* __restrict__ q_off, int nb, const int* __restrict__ q_order, int k,
                                                             int shadow, int* __restrict__ nbr_out, float* __restrict__ d2_out)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * KNN_WAVES + threadIdx.x / WAVE));
    if (t >= nq) return;
    const int qi = __builtin_amdgcn_readfirstlane(q_order ? q_order[t] : t);
    if ((unsigned)qi >= (unsigned)nq) return;                     // (not a permutation: the slot is skipped, nothing is written out of bounds)
    const int b = __builtin_amdgcn_readfirstlane(find_elem(q_off, nb, qi));
    const CellGrid g = grids[b];
    const float qx = queries[3 * (size_t)qi], qy = queries[3 * (size_t)qi + 1], qz = queries[3 * (size_t)qi + 2];
    unsigned long long mine = KNN_EMPTY, worst = KNN_EMPTY;      // lane i: the key of rank i; worst: rank k - 1 (uniform)

    const int dim[3] = { g.dim[0], g.dim[1], g.dim[2] };
    const double f[3] = { ((double)qx - (double)g.mn[0]) * g.inv_cell, ((double)qy - (double)g.mn[1]) * g.inv_cell,
                          ((double)qz - (double)g.mn[2]) * g.inv_cell };
    const int c[3] = { min(max(query_cell_coord(qx, g.mn[0], g.inv_cell, dim[0]), 0), dim[0] - 1),
                       min(max(query_cell_coord(qy, g.mn[1], g.inv_cell, dim[1]), 0), dim[1] - 1),
                       min(max(query_cell_coord(qz, g.mn[2], g.inv_cell, dim[2]), 0), dim[2] - 1) };
    // supports of this element: rows [e_lo, e_hi) of the cell-ordered array (every run below lies inside: checked, not assumed)
    const int e_lo = g.s_off;
    const int e_hi = table[g.table_off + dim[0] * dim[1] * dim[2] - 1];
    const bool searchable = isfinite(qx) && isfinite(qy) && isfinite(qz) && e_hi > e_lo;
    const int max_dim = max(dim[0], max(dim[1], dim[2]));

    for (int rho = 0; searchable && rho <= max_dim; rho++) {
        const int x0 = max(c[0] - rho, 0), x1 = min(c[0] + rho, dim[0] - 1);
        const int y0 = max(c[1] - rho, 0), y1 = min(c[1] + rho, dim[1] - 1);
        const int z0 = max(c[2] - rho, 0), z1 = min(c[2] + rho, dim[2] - 1);
        const int ny = y1 - y0 + 1;
        const long long rows = (long long)ny * (z1 - z0 + 1);   // <= the cells of the table < 2^31
        const bool xa = c[0] - rho >= 0, xb = c[0] + rho <= dim[0] - 1;
        for (long long r0 = 0; r0 < rows; r0 += WAVE) {
            // run bounds of 64 rows: a shell row is one run, an inner row its two end cells
            int s1 = 0, l1 = 0, s2 = 0, l2 = 0;
            const long long r = r0 + lane;
            if (r < rows) {
                const int y = y0 + (int)(r % ny), z = z0 + (int)(r / ny);
                const bool shell = max(abs(y - c[1]), abs(z - c[2])) == rho;
                const int rowbase = g.table_off + dim[0] * (y + dim[1] * z);
                if (shell) {
                    const int g0 = rowbase + x0;
                    s1 = g0 == 0 ? 0 : table[g0 - 1];
                    l1 = table[g0 + (x1 - x0)] - s1;
                } else {
                    if (xa) {
                        const int g0 = rowbase + x0;
                        s1 = g0 == 0 ? 0 : table[g0 - 1];
                        l1 = table[g0] - s1;
                    }
                    if (xb) {
                        const int g0 = rowbase + x1;                 // (rho >= 1 on an inner row: x1 != x0 whenever both exist)
                        s2 = table[g0 - 1];
                        l2 = table[g0] - s2;
                    }
                }
                // a run outside the element's rows would be a corrupt table: it is dropped, never read
                if (s1 < e_lo || l1 < 0 || s1 + l1 > e_hi) l1 = 0;
                if (s2 < e_lo || l2 < 0 || s2 + l2 > e_hi) l2 = 0;
            }
#pragma unroll 1
            for (int h = 0; h < 2; h++) {
                const int sv = h ? s2 : s1, lv = h ? l2 : l1;
                unsigned long long todo = __ballot(lv > 0);
                while (todo) {
                    const int j = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int rs = __builtin_amdgcn_readlane(sv, j), rl = __builtin_amdgcn_readlane(lv, j);
                    for (int p0 = 0; p0 < rl; p0 += WAVE) {
                        const bool have = p0 + lane < rl;
                        const float4 cd = have ? sorted[rs + p0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                        const float d2 = sqdist3(qx, qy, qz, cd.x, cd.y, cd.z);
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned int)__float_as_int(cd.w);
                        unsigned long long acc = __ballot(have && d2 < __builtin_inff() && key < worst);
                        while (acc) {
                            const int a = __ffsll((long long)acc) - 1;
                            acc &= acc - 1;
                            const unsigned long long ck = wave_bcast_u64(key, a);
                            if (ck < worst) {                    // (worst may have dropped since the ballot)
                                const unsigned long long up = __shfl_up(mine, 1, WAVE);
                                const bool above = mine > ck;                       // a suffix of the lanes: the row is ascending
                                const bool first = lane == 0 || !(up > ck);         // the insertion point
                                mine = above ? (first ? ck : up) : mine;
                                worst = wave_bcast_u64(mine, k - 1);
                            }
                        }
                    }
                }
            }
        }
        bool covers;
        const float bound = knn_ring_bound(f, c, dim, rho, g.inv_cell, covers);
        if (covers) break;
        if (worst != KNN_EMPTY && __uint_as_float((unsigned)(worst >> 32)) < bound) break;
    }
    if (lane < k) {
        const bool pad = mine == KNN_EMPTY;
        nbr_out[(size_t)qi * k + lane] = pad ? shadow : (int)(unsigned)(mine & 0xffffffffu);
        if (d2_out) d2_out[(size_t)qi * k + lane] = pad ? __builtin_inff() : __uint_as_float((unsigned)(mine >> 32));
    }
}

extern "C" int buf_grid_knn(const buf_grid_t* g, const float* queries, int nq, const int* q_batches_host, const int* q_order, int k,
                            int* nbr_out, float* d2_out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(g && g->ws && q_batches_host, BUF_EINVAL, "buf_grid_knn: null argument");
    BUF_REQUIRE(nq >= 0, BUF_EINVAL, "buf_grid_knn: nq=%d", nq);
    BUF_REQUIRE(k >= 1 && k <= KNN_MAX_K, BUF_EINVAL, "buf_grid_knn: k=%d (1 <= k <= %d)", k, KNN_MAX_K);
    BUF_REQUIRE(nq == 0 || queries, BUF_EINVAL, "buf_grid_knn: null queries");
    BUF_REQUIRE(nq == 0 || nbr_out, BUF_EINVAL, "buf_grid_knn: null nbr_out");
    WsCarver w(g->ws, g->ws_bytes);                      // q_off lives behind the grid in the same workspace, as in buf_grid_query
    buf_grid_t tmp;
    carve_grid(&tmp, w, g->ns, g->nb, g->cells_per_elem);
    GridExtra ex = carve_extra(w, g->ns, g->nb);
    int rc = upload_offsets(ex.q_off, q_batches_host, g->nb, nq, "buf_grid_knn", s);
    if (rc) return rc;
    if (nq == 0) return BUF_OK;
    k_grid_knn<<<cdiv(nq, KNN_WAVES), KNN_WAVES * WAVE, 0, s>>>((const CellGrid*)g->desc, g->table, (const float4*)g->sorted, queries, nq,
                                                                ex.q_off, g->nb, q_order, k, g->ns, nbr_out, d2_out);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}

// ---- N15: remove_statistical_outlier (open3d 0.13, restated; the rule stands in include/buffer_hip.h) -----------------------------
// k_outlier_row_mean: a thread per point, the fp64 sum of sqrt((double) d2) over the leading finite entries of its row, in rank order.
// k_outlier_cloud:    a workgroup per cloud.  Thread t sums the rows t, t + 256, ... of the cloud in that order; the 256 partial sums
//                     are folded by a fixed binary tree (stride 128, 64, ..., 1).  The same tree serves V, the sum of the means and
//                     the sum of the squared deviations: no atomics, the order depends on the cloud's length alone.
#define OUTL_THREADS 256

__global__ void __launch_bounds__(256) k_outlier_row_mean(const float* __restrict__ d2, int n, int k, double* __restrict__ mean_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    int cnt = 0;
    for (int j = 0; j < k; j++) {
        const float v = d2[(size_t)i * k + j];
        if (!(v < __builtin_inff())) break;               // padding (+inf) ends the row
        sum = __dadd_rn(sum, sqrt((double)v));
        cnt++;
    }
    mean_out[i] = cnt > 0 ? sum / (double)cnt : -1.0;
}

__device__ __forceinline__ double outl_tree_sum(double v, double* sh)
{
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = OUTL_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] = __dadd_rn(sh[threadIdx.x], sh[threadIdx.x + d]);
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(OUTL_THREADS) k_outlier_cloud(const double* __restrict__ mean, const int* __restrict__ off, double std_ratio,
                                                              double* __restrict__ stats_out, unsigned char* __restrict__ keep_out,
                                                              int* __restrict__ kept_out)
{
    __shared__ double sh[OUTL_THREADS];
    const int b = blockIdx.x, lo = off[b], hi = off[b + 1];
    double v = 0.0, sm = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += OUTL_THREADS) {
        const double m = mean[i];
        if (m >= 0.0) v = __dadd_rn(v, 1.0);              // a non-empty row (an empty one holds -1)
        if (m > 0.0) sm = __dadd_rn(sm, m);
    }
    const double V = outl_tree_sum(v, sh);
    const double mu = outl_tree_sum(sm, sh) / V;
    double sq = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += OUTL_THREADS) {
        const double m = mean[i];
        if (m > 0.0) { const double d = __dsub_rn(m, mu); sq = __dadd_rn(sq, __dmul_rn(d, d)); }
    }
    const double sd = sqrt(outl_tree_sum(sq, sh) / (V - 1.0));
    const double thr = __dadd_rn(mu, __dmul_rn(std_ratio, sd));
    double kept = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += OUTL_THREADS) {
        const double m = mean[i];
        const bool keep = m > 0.0 && m < thr;
        keep_out[i] = keep ? 1 : 0;
        kept += keep ? 1.0 : 0.0;
    }
    const double nk = outl_tree_sum(kept, sh);           // (a count below 2^31: exact in fp64)
    if (threadIdx.x == 0) {
        stats_out[3 * (size_t)b] = mu; stats_out[3 * (size_t)b + 1] = sd; stats_out[3 * (size_t)b + 2] = thr;
        kept_out[b] = (int)nk;
    }
}

extern "C" size_t buf_outlier_statistical_ws_bytes(int nc) { return align_up(sizeof(int) * ((size_t)(nc > 0 ? nc : 0) + 1), 256); }

extern "C" int buf_outlier_statistical(const float* d2, int n, int k, const int* lengths_host, int nc, double std_ratio, double* mean_out,
                                       double* stats_out, unsigned char* keep_out, int* kept_out, void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(n >= 0, BUF_EINVAL, "buf_outlier_statistical: n=%d", n);
    BUF_REQUIRE(k >= 1, BUF_EINVAL, "buf_outlier_statistical: k=%d", k);
    BUF_REQUIRE(nc >= 1 && nc <= 0x7ffffffe, BUF_EINVAL, "buf_outlier_statistical: nc=%d", nc);
    BUF_REQUIRE(std_ratio == std_ratio, BUF_EINVAL, "buf_outlier_statistical: std_ratio is NaN");
    BUF_REQUIRE(lengths_host && stats_out && kept_out && ws, BUF_EINVAL, "buf_outlier_statistical: null argument");
    BUF_REQUIRE(n == 0 || (d2 && mean_out && keep_out), BUF_EINVAL, "buf_outlier_statistical: null d2, mean_out or keep_out");
    BUF_REQUIRE(ws_bytes >= buf_outlier_statistical_ws_bytes(nc), BUF_EWORKSPACE, "buf_outlier_statistical: workspace %zu < %zu bytes", ws_bytes,
                buf_outlier_statistical_ws_bytes(nc));
    int rc = upload_offsets((int*)ws, lengths_host, nc, n, "buf_outlier_statistical", s);
    if (rc) return rc;
    if (n > 0) k_outlier_row_mean<<<cdiv(n, 256), 256, 0, s>>>(d2, n, k, mean_out);
    k_outlier_cloud<<<nc, OUTL_THREADS, 0, s>>>(mean_out, (const int*)ws, std_ratio, stats_out, keep_out, kept_out);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
