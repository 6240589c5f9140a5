// ICP, point-to-point, point-to-plane and Generalized (plane-to-plane), for B pairs per call (open3d registration_icp with
// TransformationEstimationPointToPoint / TransformationEstimationPointToPlane and registration_generalized_icp, restated,
// unpinned: Kabsch for point-to-point, open3d's 6x6 step for point-to-plane, the Gauss-Newton step of Segal et al. on
// normal-based covariances for Generalized ICP).  Every ICP entry point of buffer_amd/icp.py runs here.
//
// Set-up (once per call):
//   buf_grid_build   one A2 cell grid over all targets, one element per pair, radius = max_dist
//   k_icp_setup      one workgroup per pair: T <- T_init, anchor = T_init * (source centroid), state cleared
// Rounds (two launches each, no host wait between rounds):
//   k_icp_correspond one workgroup per tile of ICP_TILE source points of one pair (tile -> pair through the tile prefix
//                    offsets).  Per point: p = T s in fp64, rounded to fp32 for the search, nearest target point of the
//                    pair's grid element by the minimum 64-bit key (fp32 d2 bits, global index) with buf_grid_query's d2
//                    arithmetic and strict d2 < r2 (= column 0 of the distance-sorted query row; no sort, no row cap),
//                    non-finite points skipped.  The point's fp64 terms are summed inside the wave (xor butterfly) and
//                    across the 4 waves through LDS in a fixed order; the tile writes ONE record to the slab.
//   k_icp_update     one wave per pair: the pair's records summed in a fixed order, fitness / rmse, open3d's stopping
//                    rules, the fp64 update (Kabsch with the det correction, or the 6x6 Cholesky solve) and
//                    T <- dT T.
// No float atomics: a pair's tiles hold its own points only and every sum has a fixed order, so a pair's result does not
// depend on the other pairs of the batch and two runs give the same bits.  Finished pairs are skipped by both kernels.
// Host round trips: one int (the number of active pairs) is read back after every 8th round, so a call makes at most
// ceil((max_iteration + 1) / 8) small readbacks and no per-pair synchronisation.
#include "common.h"
#include "pose_math.h"

#define ICP_TILE 256
#define ICP_WAVES (ICP_TILE / WAVE)
#define ICP_P2P BUF_ICP_POINT_TO_POINT
#define ICP_P2L BUF_ICP_POINT_TO_PLANE
#define ICP_GICP BUF_ICP_GENERALIZED

// record values: [0] matches, [1] sum d2, then
//   point-to-point: sum P (3), sum Q (3), sum P Q^T (9, row-major) with P = p - a, Q = q - a (a = the pair's anchor)
//   point-to-plane: upper triangle of J^T J (21, row by row), J^T r (6); J = [p x n, n], r = (p - q) . n
//   generalized:    upper triangle of J^T M J (21, row by row), J^T M d (6); J = [-[p]x, I], d = p - q,
//                   M = (C(n_q) + R C(n_s) R^T)^-1 with C(n) = I - (1 - eps) n n^T
template <int M> struct IcpRec {
    static constexpr int NV = M == ICP_P2P ? 17 : 29, STRIDE = M == ICP_P2P ? 18 : 30;
    static constexpr int CNT = 0, FIT = 0, D2 = 1, H = 2, G = 23, MIN_CNT = M == ICP_P2P ? 3 : 6;     // (what pose_update reads)
    static constexpr bool KABSCH = M == ICP_P2P;
};

struct IcpState {
    double anchor[3];
    double prev_fit, prev_rmse;
    int done;
    int pad;
};

__global__ void __launch_bounds__(ICP_TILE) k_icp_setup(const float* __restrict__ src, const int* __restrict__ src_off,
                                                      const double* __restrict__ T_init, double* __restrict__ T,
                                                      double* __restrict__ fitness, double* __restrict__ rmse, int* __restrict__ iters,
                                                      IcpState* __restrict__ st)
{
    __shared__ double part[ICP_WAVES][3];
    __shared__ double cen[3];
    const int b = blockIdx.x, lo = src_off[b], n = src_off[b + 1] - lo;
    double v[3] = { 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < n; i += ICP_TILE) {
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] += (double)src[3 * (size_t)(lo + i) + c];
    }
    tile_sum<3, ICP_WAVES>(v, part, cen);
    __syncthreads();
    const double* Ti = T_init + 16 * (size_t)b;
    if (threadIdx.x < 16) T[16 * (size_t)b + threadIdx.x] = Ti[threadIdx.x];
    if (threadIdx.x == 0) {
        IcpState s;
        const double cx = n > 0 ? cen[0] / n : 0.0, cy = n > 0 ? cen[1] / n : 0.0, cz = n > 0 ? cen[2] / n : 0.0;
        for (int r = 0; r < 3; r++) {
            const double a = ((Ti[4 * r] * cx + Ti[4 * r + 1] * cy) + Ti[4 * r + 2] * cz) + Ti[4 * r + 3];
            s.anchor[r] = a == a && fabs(a) < 1e300 ? a : 0.0;            // (a non-finite centroid: NaN rows in the source)
        }
        s.prev_fit = 0.0; s.prev_rmse = 0.0; s.done = 0; s.pad = 0;
        st[b] = s;
        fitness[b] = 0.0; rmse[b] = 0.0; iters[b] = 0;
    }
}

// what only the Generalized ICP instantiation of k_icp_correspond takes (the other two have no such argument)
struct IcpGicpArgs { const float* src_normals; double w; };              // w = 1 - epsilon
__device__ __forceinline__ const IcpGicpArgs& icp_gicp_args(const IcpGicpArgs& a) { return a; }

template <int M, typename... G>
__global__ void __launch_bounds__(ICP_TILE) k_icp_correspond(const CellGrid* __restrict__ grids, const int* __restrict__ table,
                                                           const float4* __restrict__ sorted, const float* __restrict__ src,
                                                           const int* __restrict__ src_off, const int* __restrict__ tile_off, int npairs,
                                                           const float* __restrict__ tgt, const float* __restrict__ tgt_normals, int nt,
                                                           float r2, const double* __restrict__ T, const IcpState* __restrict__ st,
                                                           int* __restrict__ nn_out, double* __restrict__ slab, G... gicp)
{
    constexpr int NV = IcpRec<M>::NV;
    __shared__ double part[ICP_WAVES][NV];
    const int tile = blockIdx.x;
    const int b = find_elem(tile_off, npairs, tile);                       // uniform: a tile holds points of one pair
    if (st[b].done) return;
    const int lo = src_off[b], n = src_off[b + 1] - lo;
    const int li = (tile - tile_off[b]) * ICP_TILE + threadIdx.x;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = 0.0;
    if (li < n) {
        const size_t i = (size_t)(lo + li);
        const double* Tb = T + 16 * (size_t)b;
        const double sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
        const double px = ((Tb[0] * sx + Tb[1] * sy) + Tb[2] * sz) + Tb[3];
        const double py = ((Tb[4] * sx + Tb[5] * sy) + Tb[6] * sz) + Tb[7];
        const double pz = ((Tb[8] * sx + Tb[9] * sy) + Tb[10] * sz) + Tb[11];
        const float qx = (float)px, qy = (float)py, qz = (float)pz;      // the search runs on the fp32-rounded point
        int best = nt;
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
                        const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned int)__float_as_int(c.w);
                        key = k < key ? k : key;
                    }
                }
            }
            if (key != ~0ull) best = (int)(unsigned int)(key & 0xffffffffu);
        }
        if (nn_out) nn_out[i] = best;
        if (best < nt) {
            const double ux = tgt[3 * (size_t)best], uy = tgt[3 * (size_t)best + 1], uz = tgt[3 * (size_t)best + 2];
            const double dx = px - ux, dy = py - uy, dz = pz - uz;
            v[0] = 1.0;
            v[1] = (dx * dx + dy * dy) + dz * dz;
            if (M == ICP_P2P) {
                const double* a = st[b].anchor;
                const double P[3] = { px - a[0], py - a[1], pz - a[2] }, Q[3] = { ux - a[0], uy - a[1], uz - a[2] };
#pragma unroll
                for (int r = 0; r < 3; r++) { v[2 + r] = P[r]; v[5 + r] = Q[r]; }
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) v[8 + 3 * r + c] = P[r] * Q[c];
            } else if constexpr (M == ICP_GICP) {
                const IcpGicpArgs& ga = icp_gicp_args(gicp...);
                const double p[3] = { px, py, pz };
                double nq[3], ns[3];
                unit_normal_or_zero(tgt_normals, (size_t)best, nq);
                unit_normal_or_zero(ga.src_normals, i, ns);
                // S = C(n_q) + R C(n_s) R^T = (I - w n_q n_q^T) + (R R^T - w m m^T), m = R n_s; upper triangle 00 01 02 11 12 22
                double m[3], S[6];
#pragma unroll
                for (int r = 0; r < 3; r++) m[r] = (Tb[4 * r] * ns[0] + Tb[4 * r + 1] * ns[1]) + Tb[4 * r + 2] * ns[2];
                {
                    int k = 0;
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = r; c < 3; c++) {
                            const double rr = (Tb[4 * r] * Tb[4 * c] + Tb[4 * r + 1] * Tb[4 * c + 1]) + Tb[4 * r + 2] * Tb[4 * c + 2];
                            S[k++] = (((r == c ? 1.0 : 0.0) - ga.w * nq[r] * nq[c]) + rr) - ga.w * m[r] * m[c];
                        }
                }
                GicpTerm gt;
                gicp_term(S, p, dx, dy, dz, gt);
                int k = 2;
#pragma unroll
                for (int r = 0; r < 3; r++) {                              // rows 0..2 of H: [A^T M A | A^T M], A^T M = (M A)^T
#pragma unroll
                    for (int c = r; c < 3; c++) v[k++] = gt.AtMA[r][c];
#pragma unroll
                    for (int c = 0; c < 3; c++) v[k++] = gt.MA[c][r];
                }
#pragma unroll
                for (int r = 0; r < 3; r++)                                // rows 3..5: M
#pragma unroll
                    for (int c = r; c < 3; c++) v[k++] = gt.Mm[r][c];
#pragma unroll
                for (int r = 0; r < 3; r++) { v[23 + r] = gt.AtMd[r]; v[26 + r] = gt.Md[r]; }
            } else {
                const size_t j = 3 * (size_t)best;
                const double nx = tgt_normals[j], ny = tgt_normals[j + 1], nz = tgt_normals[j + 2];
                const double res = (dx * nx + dy * ny) + dz * nz;
                const double J[6] = { py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz };
                int k = 2;
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int c = r; c < 6; c++) v[k++] = J[r] * J[c];
#pragma unroll
                for (int r = 0; r < 6; r++) v[23 + r] = J[r] * res;
            }
        }
    }
    tile_sum<NV, ICP_WAVES>(v, part, slab + (size_t)tile * IcpRec<M>::STRIDE);
}

// One wave per pair, the update kernel of icp.hip and vgicp.hip.  Rec names the record: NV values at STRIDE, the slots CNT (terms),
// FIT (numerator of fitness) and D2 (sum of d2), the step's sums from H on (and its gradient at G), the fewest terms MIN_CNT a
// step takes, and KABSCH: the step is the Kabsch rotation about State's anchor, else the 6x6 solve.
template <class Rec, class State>
__device__ __forceinline__ void pose_update(const int* __restrict__ src_off, const int* __restrict__ tile_off,
                                            const double* __restrict__ slab, int max_iteration, double rel_fitness, double rel_rmse,
                                            double* __restrict__ T, double* __restrict__ fitness, double* __restrict__ rmse_out,
                                            int* __restrict__ iters, State* __restrict__ st, int* __restrict__ active)
{
    constexpr int NV = Rec::NV;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (st[b].done) return;
    const int t0 = tile_off[b], t1 = tile_off[b + 1];
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = 0.0;
    for (int t = t0 + lane; t < t1; t += WAVE) {
        const double* rec = slab + (size_t)t * Rec::STRIDE;
#pragma unroll
        for (int k = 0; k < NV; k++) v[k] += rec[k];
    }
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = wave_sum(v[k]);
    if (lane != 0) return;
    const int n = src_off[b + 1] - src_off[b];
    const double cnt = v[Rec::CNT];
    const double fit = n > 0 ? v[Rec::FIT] / (double)n : 0.0;
    const double rmse = cnt > 0.0 ? sqrt(v[Rec::D2] / cnt) : 0.0;
    fitness[b] = fit;
    rmse_out[b] = rmse;
    State s = st[b];
    const int it = iters[b];
    bool stop;
    double dT[4][4];
    if (it > 0 && fabs(s.prev_fit - fit) < rel_fitness && fabs(s.prev_rmse - rmse) < rel_rmse) stop = true;   // converged
    else if (it >= max_iteration) stop = true;
    else if (cnt < (double)Rec::MIN_CNT) stop = true;                                                       // too few matches
    else {
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) dT[r][c] = r == c ? 1.0 : 0.0;
        double R[9];
        if constexpr (Rec::KABSCH) {
            const double* a = s.anchor, *sp = v + Rec::H;        // sum P (3), sum Q (3), sum P Q^T (9)
            double pc[3], qc[3], H[9];
            for (int r = 0; r < 3; r++) { pc[r] = sp[r] / cnt; qc[r] = sp[3 + r] / cnt; }
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) H[3 * r + c] = sp[6 + 3 * r + c] - cnt * pc[r] * qc[c];
            stop = !kabsch_rotation(H, R);
            if (!stop) {
                const double Pa[3] = { a[0] + pc[0], a[1] + pc[1], a[2] + pc[2] }, Qa[3] = { a[0] + qc[0], a[1] + qc[1], a[2] + qc[2] };
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) dT[r][c] = R[3 * r + c];
                    dT[r][3] = Qa[r] - ((R[3 * r] * Pa[0] + R[3 * r + 1] * Pa[1]) + R[3 * r + 2] * Pa[2]);
                }
            }
        } else {
            double x[6];
            stop = !solve6(v + Rec::H, v + Rec::G, x);
            if (!stop) {
                rot_zyx(x, R);
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) dT[r][c] = R[3 * r + c];
                    dT[r][3] = x[3 + r];
                }
            }
        }
    }
    if (!stop) {
        double* Tb = T + 16 * (size_t)b;
        double Tn[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++)
                Tn[4 * r + c] = ((dT[r][0] * Tb[c] + dT[r][1] * Tb[4 + c]) + dT[r][2] * Tb[8 + c]) + dT[r][3] * Tb[12 + c];
        for (int k = 0; k < 16; k++) Tb[k] = Tn[k];
        iters[b] = it + 1;
        s.prev_fit = fit;
        s.prev_rmse = rmse;
        if (active) atomicAdd(active, 1);
    } else {
        s.done = 1;
    }
    st[b] = s;
}

template <int M>
__global__ void __launch_bounds__(WAVE) k_icp_update(const int* __restrict__ src_off, const int* __restrict__ tile_off,
                                                   const double* __restrict__ slab, int max_iteration, double rel_fitness,
                                                   double rel_rmse, double* __restrict__ T, double* __restrict__ fitness,
                                                   double* __restrict__ rmse_out, int* __restrict__ iters, IcpState* __restrict__ st,
                                                   int* __restrict__ active)
{
    pose_update<IcpRec<M>>(src_off, tile_off, slab, max_iteration, rel_fitness, rel_rmse, T, fitness, rmse_out, iters, st, active);
}

// Per-pair tile counts of tile-wide tiles as prefix offsets on the device (dst: npairs + 1 ints); the total comes back in *ntiles
static int upload_tile_offsets(int* dst, const int* lengths_host, int npairs, int tile, const char* fn, int* ntiles, hipStream_t s)
{
    int* tiles = (int*)malloc(sizeof(int) * (size_t)npairs);
    BUF_REQUIRE(tiles, BUF_EINVAL, "%s: out of host memory", fn);
    long long nts = 0;
    for (int b = 0; b < npairs; b++) nts += tiles[b] = cdiv(lengths_host[b], tile);
    const int rc = upload_offsets(dst, tiles, npairs, (int)nts, fn, s);
    free(tiles);
    *ntiles = (int)nts;
    return rc;
}

// The rounds of icp.hip and vgicp.hip on the workspace e (src_off, tile_off, slab, st, active): launch_terms() puts the kernel that writes the records on the stream, update is the
// k_*_update entry point.  One int (the pairs still active) is read back after every 8th round.
template <class Ws, class State, class Terms>
static int pose_rounds(const Ws& e, Terms launch_terms, void (*update)(const int*, const int*, const double*, int, double, double, double*,
                                                                       double*, double*, int*, State*, int*),
                       int npairs, int max_iteration, double rel_fitness, double rel_rmse, double* T_out, double* fitness_out,
                       double* rmse_out, int* iters_out, hipStream_t s)
{
    for (int r = 0; r <= max_iteration; r++) {
        const bool probe = (r & 7) == 7 && r < max_iteration;
        if (probe) BUF_CHECK_HIP(hipMemsetAsync(e.active, 0, sizeof(int), s));
        launch_terms();
        update<<<npairs, WAVE, 0, s>>>(e.src_off, e.tile_off, e.slab, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out,
                                       iters_out, e.st, probe ? e.active : nullptr);
        if (probe) {
            BUF_LAUNCH_CHECK();
            int left = 0;
            BUF_CHECK_HIP(hipMemcpyAsync(&left, e.active, sizeof(int), hipMemcpyDeviceToHost, s));
            BUF_CHECK_HIP(hipStreamSynchronize(s));
            if (left == 0) break;
        }
    }
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}

// ------------------------------------------------------------------------------------------
static int icp_tiles_upper(int n_src_total, int npairs) { return cdiv(n_src_total, ICP_TILE) + npairs; }

struct IcpWs { void* grid; size_t grid_bytes; int* src_off; int* tile_off; IcpState* st; double* slab; int* active; };

static IcpWs carve_icp(WsCarver& w, int ns, int nt, int npairs, int method)
{
    IcpWs e;
    e.grid_bytes = buf_grid_ws_bytes(nt, npairs, 0);
    e.grid = w.take<char>(e.grid_bytes);
    e.src_off = w.take<int>((size_t)npairs + 1);
    e.tile_off = w.take<int>((size_t)npairs + 1);
    e.st = w.take<IcpState>((size_t)npairs);
    e.slab = w.take<double>((size_t)icp_tiles_upper(ns, npairs) *
                            (method == ICP_P2P ? IcpRec<ICP_P2P>::STRIDE : IcpRec<ICP_P2L>::STRIDE));
    e.active = w.take<int>(64);
    return e;
}

extern "C" size_t buf_icp_ws_bytes(int n_src_total, int n_tgt_total, int npairs, int method)
{
    if (n_src_total < 0 || n_tgt_total < 0 || npairs <= 0 || (method != ICP_P2P && method != ICP_P2L && method != ICP_GICP)) return 0;
    WsCarver w(nullptr, 0);
    carve_icp(w, n_src_total, n_tgt_total, npairs, method);
    return w.used();
}

template <int M, typename... G>
static int icp_rounds(const IcpWs& e, const buf_grid_t& g, const float* src, const float* tgt, const float* tgt_normals, int nt,
                      int npairs, int ntiles, float r2, int max_iteration, double rel_fitness, double rel_rmse, double* T_out,
                      double* fitness_out, double* rmse_out, int* iters_out, int* nn_out, hipStream_t s, G... gicp)
{
    const auto terms = [&] {
        if (ntiles > 0)
            k_icp_correspond<M><<<ntiles, ICP_TILE, 0, s>>>((const CellGrid*)g.desc, g.table, (const float4*)g.sorted, src, e.src_off,
                                                           e.tile_off, npairs, tgt, tgt_normals, nt, r2, T_out, e.st, nn_out, e.slab,
                                                           gicp...);
    };
    return pose_rounds(e, terms, k_icp_update<M>, npairs, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out, iters_out, s);
}

// buf_icp_batched (fn = its name, method 0 / 1) and buf_gicp_batched (method 2, with src_normals and epsilon): one body
static int icp_run(const char* fn, const float* src, const float* src_normals, const int* src_lengths_host, const float* tgt,
                   const float* tgt_normals, const int* tgt_lengths_host, int npairs, int method, float max_dist, double epsilon,
                   const double* T_init, int max_iteration, double rel_fitness, double rel_rmse, double* T_out, double* fitness_out,
                   double* rmse_out, int* iters_out, int* nn_out, void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(npairs >= 0, BUF_EINVAL, "%s: npairs=%d", fn, npairs);
    BUF_REQUIRE(max_dist > 0.f && max_dist <= 3.4e38f, BUF_EINVAL, "%s: max_dist=%g (must be finite and > 0)", fn, (double)max_dist);
    BUF_REQUIRE(method != ICP_P2L || tgt_normals, BUF_EINVAL, "%s: point-to-plane needs target normals", fn);
    BUF_REQUIRE(method != ICP_GICP || (epsilon > 0.0 && epsilon <= 1.0), BUF_EINVAL, "%s: epsilon=%g (must be in (0, 1])", fn, epsilon);
    BUF_REQUIRE(max_iteration >= 0, BUF_EINVAL, "%s: max_iteration=%d", fn, max_iteration);
    if (npairs == 0) return BUF_OK;
    BUF_REQUIRE(src_lengths_host && tgt_lengths_host, BUF_EINVAL, "%s: null lengths", fn);
    long long ns = 0, nt = 0;
    for (int b = 0; b < npairs; b++) {
        BUF_REQUIRE(src_lengths_host[b] >= 0 && tgt_lengths_host[b] >= 0, BUF_EINVAL, "%s: negative length in pair %d", fn, b);
        ns += src_lengths_host[b];
        nt += tgt_lengths_host[b];
    }
    BUF_REQUIRE(ns < 0x7fffffffLL && nt < 0x7fffffffLL, BUF_EINVAL, "%s: %lld / %lld points (int32 indices)", fn, ns, nt);
    BUF_REQUIRE(ns == 0 || src, BUF_EINVAL, "%s: null src", fn);
    BUF_REQUIRE(nt == 0 || tgt, BUF_EINVAL, "%s: null tgt", fn);
    BUF_REQUIRE(method != ICP_GICP || ((ns == 0 || src_normals) && (nt == 0 || tgt_normals)), BUF_EINVAL,
                "%s: Generalized ICP needs source and target normals", fn);
    BUF_REQUIRE(T_init && T_out && fitness_out && rmse_out && iters_out && ws, BUF_EINVAL, "%s: null argument", fn);
    BUF_REQUIRE(npairs <= 65535, BUF_EINVAL, "%s: %d pairs (at most 65535 per call)", fn, npairs);
    const size_t need = buf_icp_ws_bytes((int)ns, (int)nt, npairs, method);
    BUF_REQUIRE(ws_bytes >= need, BUF_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);

    WsCarver w(ws, ws_bytes);
    const IcpWs e = carve_icp(w, (int)ns, (int)nt, npairs, method);
    buf_grid_t g;
    int rc = buf_grid_build(&g, tgt, (int)nt, tgt_lengths_host, npairs, max_dist, 0, e.grid, e.grid_bytes, s);
    if (rc) return rc;
    rc = upload_offsets(e.src_off, src_lengths_host, npairs, (int)ns, fn, s);
    if (rc) return rc;
    int nts = 0;
    rc = upload_tile_offsets(e.tile_off, src_lengths_host, npairs, ICP_TILE, fn, &nts, s);
    if (rc) return rc;
    k_icp_setup<<<npairs, ICP_TILE, 0, s>>>(src, e.src_off, T_init, T_out, fitness_out, rmse_out, iters_out, e.st);
    BUF_LAUNCH_CHECK();
    const float r2 = max_dist * max_dist;                 // buf_grid_query's threshold
    if (method == ICP_P2P)
        return icp_rounds<ICP_P2P>(e, g, src, tgt, nullptr, (int)nt, npairs, nts, r2, max_iteration, rel_fitness, rel_rmse, T_out,
                                   fitness_out, rmse_out, iters_out, nn_out, s);
    if (method == ICP_P2L)
        return icp_rounds<ICP_P2L>(e, g, src, tgt, tgt_normals, (int)nt, npairs, nts, r2, max_iteration, rel_fitness, rel_rmse, T_out,
                                   fitness_out, rmse_out, iters_out, nn_out, s);
    return icp_rounds<ICP_GICP>(e, g, src, tgt, tgt_normals, (int)nt, npairs, nts, r2, max_iteration, rel_fitness, rel_rmse, T_out,
                                fitness_out, rmse_out, iters_out, nn_out, s, IcpGicpArgs{ src_normals, 1.0 - epsilon });
}

extern "C" int buf_icp_batched(const float* src, const int* src_lengths_host, const float* tgt, const float* tgt_normals,
                               const int* tgt_lengths_host, int npairs, int method, float max_dist, const double* T_init,
                               int max_iteration, double rel_fitness, double rel_rmse, double* T_out, double* fitness_out,
                               double* rmse_out, int* iters_out, int* nn_out, void* ws, size_t ws_bytes, void* stream)
{
    // (Generalized ICP has its own entry: this one has no source normals to give it)
    BUF_REQUIRE(method == ICP_P2P || method == ICP_P2L, BUF_EINVAL, "buf_icp_batched: unknown method %d", method);
    return icp_run("buf_icp_batched", src, nullptr, src_lengths_host, tgt, tgt_normals, tgt_lengths_host, npairs, method, max_dist, 1.0,
                   T_init, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out, iters_out, nn_out, ws, ws_bytes, stream);
}

extern "C" int buf_gicp_batched(const float* src, const float* src_normals, const int* src_lengths_host, const float* tgt,
                                const float* tgt_normals, const int* tgt_lengths_host, int npairs, float max_dist, double epsilon,
                                const double* T_init, int max_iteration, double rel_fitness, double rel_rmse, double* T_out,
                                double* fitness_out, double* rmse_out, int* iters_out, int* nn_out, void* ws, size_t ws_bytes,
                                void* stream)
{
    return icp_run("buf_gicp_batched", src, src_normals, src_lengths_host, tgt, tgt_normals, tgt_lengths_host, npairs, ICP_GICP, max_dist,
                   epsilon, T_init, max_iteration, rel_fitness, rel_rmse, T_out, fitness_out, rmse_out, iters_out, nn_out, ws, ws_bytes,
                   stream);
}
