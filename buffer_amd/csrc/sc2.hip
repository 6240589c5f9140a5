// N8  SC2-PCR (Chen, Sun, Yang, Tao, CVPR 2022: second order spatial compatibility), the single-stage form restated from its
// published form, unpinned: no other implementation was at hand, the contract is in include/buffer_hip.h.  B pairs per call,
// 8 + power_iterations launches, nothing read back.
//
//   k_sc2_gather   one lane per correspondence row: the two points promoted to fp64, the live flag; seeds and counts reset to -1
//   k_sc2_compat   tile of 64 rows x 256 columns per workgroup.  A wavefront owns one 64-bit word column: lane = column, the 64 row
//                  points come from LDS, the ballot of e_ij <= d_thr over the wavefront IS the word (row i, word j / 64) of the bit
//                  matrix C (n x ceil(n / 64) words per pair).  Only C is kept: neither e nor the soft values are stored.
//   k_sc2_power    one step v <- S (v / max v): lane = row, the columns' points and confidences are staged in LDS tiles and a lane
//                  walks the SET bits of its own row in ascending column order (s_ij is exactly 0 where the bit is clear, and adding
//                  +0 changes nothing): the cost of the compatible pairs only.  The four wavefronts of a workgroup share 64 rows and
//                  deal the column tiles among themselves; a row's four partial sums are added in a fixed tree.  The
//                  max-normalisation of a step is applied by the next reader (a maximum has no order).
//   k_sc2_conf     the last normalisation, conf_out and the non-maximum suppression (same staging)
//   k_sc2_seeds    lane = row: its place among all rows by (confidence descending, row ascending); the first S places are the seeds
//   k_sc2_counts   16 seed rows of C in LDS, lane = column: its row of C is streamed once and ANDed with all 16 (popcount), masked by
//                  the column's bit in the seed row.  Integers: exact.  (A matrix-pipe form was not built: see DESIGN.md.)
//   k_sc2_hyp      one wavefront per seed: the k1 largest counts (k1 passes of a wavefront maximum over packed (count, column)
//                  keys: descending count, ascending column), the power iteration on the set's soft submatrix (lane = row,
//                  ascending columns), the weighted Kabsch pose and its inlier count over all live rows
//   k_sc2_refine   one workgroup per pair: the winner, the refits over its inliers, every output
// All fp64 without FMA (the library is built with -ffp-contract=off); no atomics and a fixed order in every sum: a pair's outputs
// are the same bits alone, in any batch and across runs.
#include "common.h"
#include "pose_math.h"

#define SC2_W 256
#define SC2_WAVES (SC2_W / WAVE)
#define SC2_MAX_WORDS (BUF_SC2_MAX_ROWS / 64)
#define SC2_TC 128                                               // columns per LDS tile of the lane-per-row kernels
#define SC2_SG 16                                                // seed rows per workgroup of k_sc2_counts
#define SC2_MAX_K1 128
#define SC2_MAX_SEEDS 1024
#define SC2_MAX_PAIRS 65535                                      // (the pair is a grid dimension)

struct Sc2Pair { int src_off, ns, tgt_off, nt, corr_off, n, S, pad; long long bits_off, cnt_off; };
#define SC2_PAIR_INTS ((int)(sizeof(Sc2Pair) / sizeof(int)))

__device__ __forceinline__ double sc2_dist(const double* a, const double* b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// e_ij of two rows r = (p | q), 6 doubles each
__device__ __forceinline__ double sc2_err(const double* ri, const double* rj)
{
    return fabs(sc2_dist(ri, rj) - sc2_dist(ri + 3, rj + 3));
}

__device__ __forceinline__ double sc2_soft(double e, double d2)
{
    const double s = 1.0 - (e * e) / d2;
    return s > 0.0 ? s : 0.0;
}

__device__ __forceinline__ double sc2_wave_max(double v)
{
    for (int d = WAVE / 2; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, WAVE));
    return v;
}

__device__ __forceinline__ unsigned long long sc2_wave_max_u64(unsigned long long v)
{
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

// |R p + t - q| of a row r = (p | q) under T = [R (9, row-major) | t (3)]
__device__ __forceinline__ double sc2_residual(const double* T, const double* r)
{
    const double x = (((T[0] * r[0] + T[1] * r[1]) + T[2] * r[2]) + T[9]) - r[3];
    const double y = (((T[3] * r[0] + T[4] * r[1]) + T[5] * r[2]) + T[10]) - r[4];
    const double z = (((T[6] * r[0] + T[7] * r[1]) + T[8] * r[2]) + T[11]) - r[5];
    return sqrt((x * x + y * y) + z * z);
}

// T = [R | cq - R cp] from the centroids and H (the identity rotation where H is zero or not finite)
__device__ static void sc2_pose(const double* cp, const double* cq, const double* H, double* T)
{
    double R[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
    if (finite9(H)) kabsch_rotation(H, R);
    for (int k = 0; k < 9; k++) T[k] = R[k];
    for (int r = 0; r < 3; r++) T[9 + r] = cq[r] - ((R[3 * r] * cp[0] + R[3 * r + 1] * cp[1]) + R[3 * r + 2] * cp[2]);
}

// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SC2_W) k_sc2_gather(const float* __restrict__ src, const float* __restrict__ tgt,
                                                    const int* __restrict__ corr, const Sc2Pair* __restrict__ mp, int max_seeds,
                                                    double* __restrict__ rows, int* __restrict__ live, int* __restrict__ seeds,
                                                    int* __restrict__ hypc)
{
    const Sc2Pair P = mp[blockIdx.y];
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < max_seeds; k += SC2_W) {
            seeds[(size_t)blockIdx.y * max_seeds + k] = -1;
            hypc[(size_t)blockIdx.y * max_seeds + k] = -1;
        }
    const int i = blockIdx.x * SC2_W + threadIdx.x;
    if (i >= P.n) return;
    const size_t g = (size_t)P.corr_off + i;
    const int is = corr[2 * g], it = corr[2 * g + 1];
    bool ok = (unsigned int)is < (unsigned int)P.ns && (unsigned int)it < (unsigned int)P.nt;
    double r[6];
    for (int c = 0; c < 3; c++) {
        r[c] = ok ? (double)src[3 * ((size_t)P.src_off + is) + c] : 0.0;
        r[3 + c] = ok ? (double)tgt[3 * ((size_t)P.tgt_off + it) + c] : 0.0;
    }
    for (int c = 0; c < 6; c++) ok = ok && isfinite(r[c]);
    for (int c = 0; c < 6; c++) rows[6 * g + c] = ok ? r[c] : 0.0;
    live[g] = ok ? 1 : 0;
}

// grid (word columns / 4, row tiles of 64, pairs)
__global__ void __launch_bounds__(SC2_W) k_sc2_compat(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                    const int* __restrict__ live, double d_thr, unsigned long long* __restrict__ bits)
{
    __shared__ double rr[WAVE][6];
    __shared__ int rl[WAVE];
    const Sc2Pair P = mp[blockIdx.z];
    const int n = P.n, W = (n + 63) >> 6, r0 = blockIdx.y * WAVE, tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    if (r0 >= n || (int)blockIdx.x * SC2_WAVES >= W) return;     // (block-uniform)
    if (tid < WAVE) {
        const int i = r0 + tid;
        const bool in = i < n;
        rl[tid] = in ? live[(size_t)P.corr_off + i] : 0;
        for (int c = 0; c < 6; c++) rr[tid][c] = in ? rows[6 * ((size_t)P.corr_off + i) + c] : 0.0;
    }
    __syncthreads();
    const int wc = blockIdx.x * SC2_WAVES + wave;
    if (wc >= W) return;                                         // (wavefront-uniform, after the only barrier)
    const int j = wc * WAVE + lane;
    const bool cl = j < n && live[(size_t)P.corr_off + (j < n ? j : 0)] != 0;
    double cr[6];
    for (int c = 0; c < 6; c++) cr[c] = cl ? rows[6 * ((size_t)P.corr_off + j) + c] : 0.0;
    unsigned long long mine = 0ull;
    for (int r = 0; r < WAVE; r++) {
        if (!rl[r]) continue;                                    // (uniform: a dead row keeps its zero word)
        const unsigned long long m = __ballot(cl && sc2_err(rr[r], cr) <= d_thr);
        if (lane == r) mine = m;
    }
    if (r0 + lane < n) bits[P.bits_off + (long long)(r0 + lane) * W + wc] = mine;
}

// the columns c0 .. c0 + cnt - 1 of a pair into an LDS tile: the rows (p | q) and val = live ? v / mx : dead
__device__ __forceinline__ void sc2_stage(const Sc2Pair& P, const double* __restrict__ rows, const int* __restrict__ live,
                                          const double* __restrict__ v, double mx, double dead, int c0, int cnt, double (*tr)[6], double* tv)
{
    for (int t = threadIdx.x % WAVE; t < cnt; t += WAVE) {
        const size_t g = (size_t)P.corr_off + c0 + t;
        for (int c = 0; c < 6; c++) tr[t][c] = rows[6 * g + c];
        tv[t] = live[g] ? (v ? v[g] / mx : 1.0) : dead;
    }
}

// max of v over the live rows of a pair (v == nullptr: the start vector of ones), in every lane
__device__ __forceinline__ double sc2_pair_max(const Sc2Pair& P, const int* __restrict__ live, const double* __restrict__ v)
{
    if (!v) return 1.0;
    double mx = 0.0;
    for (int j = threadIdx.x % WAVE; j < P.n; j += WAVE)
        if (live[(size_t)P.corr_off + j]) mx = fmax(mx, v[(size_t)P.corr_off + j]);
    return sc2_wave_max(mx);
}

// grid (row tiles of 64, pairs): vout = S (vin / max vin).  The four wavefronts of a workgroup share its 64 rows: column tile t
// (SC2_TC columns) belongs to wavefront t % 4, which stages it in its own LDS tile and adds it to its own partial sum; the row's value
// is (s0 + s1) + (s2 + s3).
__global__ void __launch_bounds__(SC2_W) k_sc2_power(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                   const int* __restrict__ live, const unsigned long long* __restrict__ bits, double d2,
                                                   const double* __restrict__ vin, double* __restrict__ vout)
{
    __shared__ double tr[SC2_WAVES][SC2_TC][6];
    __shared__ double tv[SC2_WAVES][SC2_TC];
    __shared__ double part[SC2_WAVES][WAVE];
    const Sc2Pair P = mp[blockIdx.y];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int n = P.n, W = (n + 63) >> 6, i = blockIdx.x * WAVE + lane;
    if ((int)blockIdx.x * WAVE >= n) return;                     // (block-uniform)
    const double mx = sc2_pair_max(P, live, vin);
    const bool li = i < n && live[(size_t)P.corr_off + (i < n ? i : 0)] != 0;
    double me[6];
    for (int c = 0; c < 6; c++) me[c] = li ? rows[6 * ((size_t)P.corr_off + i) + c] : 0.0;
    const unsigned long long* brow = bits + P.bits_off + (long long)(li ? i : 0) * W;
    double acc = 0.0;
    for (int c0 = wave * SC2_TC; c0 < n; c0 += SC2_WAVES * SC2_TC) {
        const int cnt = n - c0 < SC2_TC ? n - c0 : SC2_TC;
        wave_sync();
        sc2_stage(P, rows, live, vin, mx, 0.0, c0, cnt, tr[wave], tv[wave]);
        wave_sync();
        if (!li) continue;
        for (int w = c0 >> 6; w < W && w < ((c0 + SC2_TC) >> 6); w++) {
            unsigned long long m = brow[w];
            while (m) {
                const int j = ((w << 6) - c0) + (__ffsll((long long)m) - 1);
                m &= m - 1ull;
                acc += sc2_soft(sc2_err(me, tr[wave][j]), d2) * tv[wave][j];
            }
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && i < n) vout[(size_t)P.corr_off + i] = li ? (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]) : 0.0;
}

// grid (row tiles of 64, pairs): conf = v / max v, conf_out, and the suppressed confidence c (-1: dead or suppressed)
__global__ void __launch_bounds__(WAVE) k_sc2_conf(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                 const int* __restrict__ live, const double* __restrict__ vin, double nms_radius,
                                                 double* __restrict__ c_out, double* __restrict__ conf_out)
{
    __shared__ double tr[SC2_TC][6];
    __shared__ double tv[SC2_TC];
    const Sc2Pair P = mp[blockIdx.y];
    const int n = P.n, i = blockIdx.x * WAVE + threadIdx.x;
    if ((int)blockIdx.x * WAVE >= n) return;
    const double mx = sc2_pair_max(P, live, vin);
    const size_t g = (size_t)P.corr_off + (i < n ? i : 0);
    const bool li = i < n && live[g] != 0;
    const double conf = li ? (vin ? vin[g] / mx : 1.0) : -1.0;
    bool keep = li;
    if (nms_radius > 0.0) {
        double me[3];
        for (int c = 0; c < 3; c++) me[c] = rows[6 * g + c];
        for (int c0 = 0; c0 < n; c0 += SC2_TC) {
            const int cnt = n - c0 < SC2_TC ? n - c0 : SC2_TC;
            __syncthreads();
            sc2_stage(P, rows, live, vin, mx, -1.0, c0, cnt, tr, tv);
            __syncthreads();
            if (!li) continue;
            for (int j = 0; j < cnt; j++)                        // (a dead column holds -1: never above a live confidence)
                if (tv[j] > conf && sc2_dist(me, tr[j]) <= nms_radius) keep = false;
        }
    }
    if (i < n) {
        c_out[g] = keep ? conf : -1.0;
        if (conf_out) conf_out[g] = li ? conf : __builtin_nan("");
    }
}

// grid (row tiles of 64, pairs): seeds[place] = row for the rows with c > 0 whose place is below S
__global__ void __launch_bounds__(WAVE) k_sc2_seeds(const Sc2Pair* __restrict__ mp, const double* __restrict__ c, int max_seeds,
                                                  int* __restrict__ seeds)
{
    const Sc2Pair P = mp[blockIdx.y];
    const int n = P.n, i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const double* cp = c + P.corr_off;
    const double ci = cp[i];
    if (!(ci > 0.0)) return;
    int place = 0;
    for (int j = 0; j < n; j++) {
        const double cj = cp[j];
        place += (cj > ci || (cj == ci && j < i)) ? 1 : 0;
    }
    if (place < P.S) seeds[(size_t)blockIdx.y * max_seeds + place] = i;
}

__global__ void __launch_bounds__(SC2_W) k_sc2_fill(int* __restrict__ p, long long n, int v)
{
    for (long long i = (long long)blockIdx.x * SC2_W + threadIdx.x; i < n; i += (long long)gridDim.x * SC2_W) p[i] = v;
}

// grid (column tiles of 256, seed groups of 16, pairs): K[rank, j] = C[s, j] * popcount(row_s AND row_j); -1 on a rank without a seed.
// counts_out == nullptr: into the workspace (pair block at cnt_off), else into counts_out (pair block at max_seeds * corr_off).
__global__ void __launch_bounds__(SC2_W) k_sc2_counts(const Sc2Pair* __restrict__ mp, const unsigned long long* __restrict__ bits,
                                                    const int* __restrict__ seeds, int max_seeds, int* __restrict__ counts_ws,
                                                    int* __restrict__ counts_out)
{
    __shared__ unsigned long long srow[SC2_SG][SC2_MAX_WORDS];
    __shared__ int sidx[SC2_SG];
    const Sc2Pair P = mp[blockIdx.z];
    const int n = P.n, W = (n + 63) >> 6, j0 = blockIdx.x * SC2_W, g0 = blockIdx.y * SC2_SG, tid = threadIdx.x;
    if (j0 >= n || g0 >= P.S) return;                            // (block-uniform)
    if (tid < SC2_SG) sidx[tid] = g0 + tid < P.S ? seeds[(size_t)blockIdx.z * max_seeds + g0 + tid] : -1;
    __syncthreads();
    const unsigned long long* B = bits + P.bits_off;
    for (int t = tid; t < SC2_SG * W; t += SC2_W) {
        const int s = t / W, w = t - s * W;
        srow[s][w] = sidx[s] >= 0 ? B[(long long)sidx[s] * W + w] : 0ull;
    }
    __syncthreads();
    const int j = j0 + tid;
    if (j >= n) return;
    int acc[SC2_SG];
#pragma unroll
    for (int s = 0; s < SC2_SG; s++) acc[s] = 0;
    const unsigned long long* brow = B + (long long)j * W;
    for (int w = 0; w < W; w++) {
        const unsigned long long x = brow[w];
#pragma unroll
        for (int s = 0; s < SC2_SG; s++) acc[s] += __popcll(x & srow[s][w]);
    }
    int* out = counts_out ? counts_out + (long long)max_seeds * P.corr_off : counts_ws + P.cnt_off;
#pragma unroll
    for (int s = 0; s < SC2_SG; s++) {
        const int r = g0 + s;
        if (r >= P.S) break;
        const int k = sidx[s] < 0 ? -1 : (((srow[s][j >> 6] >> (j & 63)) & 1ull) ? acc[s] : 0);
        out[(long long)r * n + j] = k;
    }
}

// grid (seed ranks, pairs), one wavefront per seed
__global__ void __launch_bounds__(WAVE) k_sc2_hyp(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                const int* __restrict__ live, const int* __restrict__ seeds, int max_seeds,
                                                const int* __restrict__ counts_ws, const int* __restrict__ counts_out, int k1, double d2,
                                                int power_iterations, double inlier_thr, int* __restrict__ hypc, double* __restrict__ hypT)
{
    __shared__ double sr[SC2_MAX_K1][6];
    __shared__ double sw[2][SC2_MAX_K1];
    __shared__ int member[SC2_MAX_K1];
    const Sc2Pair P = mp[blockIdx.y];
    const int n = P.n, rank = blockIdx.x, lane = threadIdx.x;
    if (rank >= P.S) return;
    const size_t slot = (size_t)blockIdx.y * max_seeds + rank;
    if (seeds[slot] < 0) return;                                 // (hypc holds -1 from k_sc2_gather)
    const int* K = (counts_out ? counts_out + (long long)max_seeds * P.corr_off : counts_ws + P.cnt_off) + (long long)rank * n;

    // the k1 largest counts: keys (count << 32 | ~column) are distinct, each pass takes the largest key below the last one
    int m = 0;
    unsigned long long prev = ~0ull;
    for (int t = 0; t < k1; t++) {
        unsigned long long best = 0ull;
        for (int j = lane; j < n; j += WAVE) {
            const int kv = K[j];
            const unsigned long long key = ((unsigned long long)(unsigned int)kv << 32) | (unsigned long long)(0xffffffffu - (unsigned int)j);
            if (kv > 0 && key < prev && key > best) best = key;
        }
        best = sc2_wave_max_u64(best);
        if (best == 0ull) break;
        if (lane == 0) member[m] = (int)(0xffffffffu - (unsigned int)(best & 0xffffffffull));
        m++;
        prev = best;
    }
    if (m < 3) return;
    __syncthreads();
    for (int a = lane; a < m; a += WAVE) {
        for (int c = 0; c < 6; c++) sr[a][c] = rows[6 * ((size_t)P.corr_off + member[a]) + c];
        sw[0][a] = 1.0;
    }
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < power_iterations; it++) {
        double mx = 0.0, nv[SC2_MAX_K1 / WAVE];
#pragma unroll
        for (int h = 0; h < SC2_MAX_K1 / WAVE; h++) {
            const int a = lane + h * WAVE;
            double acc = 0.0;
            if (a < m)
                for (int j = 0; j < m; j++) acc += sc2_soft(sc2_err(sr[a], sr[j]), d2) * sw[cur][j];
            nv[h] = acc;
            mx = fmax(mx, acc);
        }
        mx = sc2_wave_max(mx);
#pragma unroll
        for (int h = 0; h < SC2_MAX_K1 / WAVE; h++)
            if (lane + h * WAVE < m) sw[cur ^ 1][lane + h * WAVE] = nv[h] / mx;
        cur ^= 1;
        __syncthreads();
    }
    // weighted Kabsch on the normalised weights
    double part = 0.0;
    for (int a = lane; a < m; a += WAVE) part += sw[cur][a];
    const double wsum = wave_sum(part);
    double cen[6], H[9];
    for (int c = 0; c < 6; c++) {
        part = 0.0;
        for (int a = lane; a < m; a += WAVE) part += (sw[cur][a] / wsum) * sr[a][c];
        cen[c] = wave_sum(part);
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            part = 0.0;
            for (int a = lane; a < m; a += WAVE) part += (sw[cur][a] / wsum) * ((sr[a][r] - cen[r]) * (sr[a][3 + c] - cen[3 + c]));
            H[3 * r + c] = wave_sum(part);
        }
    double T[12];
    sc2_pose(cen, cen + 3, H, T);                                // (every lane holds the same sums: the same pose in every lane)
    int count = 0;
    for (int j0 = 0; j0 < n; j0 += WAVE) {
        const int j = j0 + lane;
        bool in = false;
        if (j < n && live[(size_t)P.corr_off + j]) in = sc2_residual(T, rows + 6 * ((size_t)P.corr_off + j)) < inlier_thr;
        count += __popcll(__ballot(in));
    }
    if (lane == 0) {
        hypc[slot] = count;
        for (int k = 0; k < 12; k++) hypT[12 * slot + k] = T[k];
    }
}

// The refits of T over its inliers (live rows with a residual below inlier_thr) by one workgroup of SC2_W: sums, centroids, H,
// pose, until the count stops growing or falls below 3.  Block-uniform: every thread holds the same T and counts.
__device__ static void sc2_refit(const double* __restrict__ R, const int* __restrict__ L, int n, double inlier_thr, int refine_iterations,
                                 double* red, double* T)
{
    const int tid = threadIdx.x;
    int last = 0;
    for (int it = 0; it < refine_iterations; it++) {
        double s[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        for (int i = tid; i < n; i += SC2_W)
            if (L[i] && sc2_residual(T, R + 6 * (size_t)i) < inlier_thr) {
                for (int c = 0; c < 6; c++) s[c] += R[6 * (size_t)i + c];
                s[6] += 1.0;
            }
        tile_sum<7, SC2_WAVES>(s, red);
        const int count = (int)s[6];
        if ((it > 0 && count <= last) || count < 3) break;
        last = count;
        double cen[6], H[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        for (int c = 0; c < 6; c++) cen[c] = s[c] / s[6];
        for (int i = tid; i < n; i += SC2_W)
            if (L[i] && sc2_residual(T, R + 6 * (size_t)i) < inlier_thr)
                for (int r = 0; r < 3; r++)
                    for (int c = 0; c < 3; c++) H[3 * r + c] += (R[6 * (size_t)i + r] - cen[r]) * (R[6 * (size_t)i + 3 + c] - cen[3 + c]);
        tile_sum<9, SC2_WAVES>(H, red);
        sc2_pose(cen, cen + 3, H, T);
    }
}

// one workgroup per pair
__global__ void __launch_bounds__(SC2_W) k_sc2_refine(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                    const int* __restrict__ live, const int* __restrict__ seeds, int max_seeds,
                                                    const int* __restrict__ hypc, const double* __restrict__ hypT, double inlier_thr,
                                                    int refine_iterations, double* __restrict__ T_out, int* __restrict__ info,
                                                    int* __restrict__ seeds_out, int* __restrict__ hyp_counts_out,
                                                    unsigned char* __restrict__ inliers_out)
{
    __shared__ double red[SC2_WAVES * 9];
    __shared__ unsigned long long wbest[SC2_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Sc2Pair P = mp[b];
    const int n = P.n;
    const double* R = rows + 6 * (size_t)P.corr_off;
    const int* L = live + P.corr_off;
    const int* sd = seeds + (size_t)b * max_seeds, *hc = hypc + (size_t)b * max_seeds;

    // live rows, seeds, the winner (largest count, then lowest rank)
    double cnt2[2] = { 0.0, 0.0 };                               // (counts below 2^53: exact in fp64)
    for (int i = tid; i < n; i += SC2_W) cnt2[0] += L[i] ? 1.0 : 0.0;
    unsigned long long best = 0ull;
    for (int r = tid; r < P.S; r += SC2_W) {
        cnt2[1] += sd[r] >= 0 ? 1.0 : 0.0;
        if (hc[r] >= 0) {
            const unsigned long long key = ((unsigned long long)(unsigned int)(hc[r] + 1) << 32) | (unsigned long long)(0xffffffffu - (unsigned int)r);
            best = key > best ? key : best;
        }
    }
    tile_sum<2, SC2_WAVES>(cnt2, red);
    best = sc2_wave_max_u64(best);
    if (tid % WAVE == 0) wbest[tid / WAVE] = best;
    __syncthreads();
    best = 0ull;
    for (int w = 0; w < SC2_WAVES; w++) best = wbest[w] > best ? wbest[w] : best;
    const int n_live = (int)cnt2[0], n_seeds = (int)cnt2[1];
    const int win = best ? (int)(0xffffffffu - (unsigned int)(best & 0xffffffffull)) : -1;
    const int win_count = best ? (int)(best >> 32) - 1 : 0;
    const bool ok = n_live >= 3 && win >= 0 && win_count >= 3;

    double T[12];
    for (int k = 0; k < 12; k++) T[k] = ok ? hypT[12 * ((size_t)b * max_seeds + win) + k] : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
    if (ok) sc2_refit(R, L, n, inlier_thr, refine_iterations, red, T);
    double fin[1] = { 0.0 };
    for (int i = tid; i < n; i += SC2_W) {
        const bool in = ok && L[i] && sc2_residual(T, R + 6 * (size_t)i) < inlier_thr;
        fin[0] += in ? 1.0 : 0.0;
        if (inliers_out) inliers_out[(size_t)P.corr_off + i] = in ? 1 : 0;
    }
    tile_sum<1, SC2_WAVES>(fin, red);
    for (int k = tid; k < max_seeds; k += SC2_W) {
        if (seeds_out) seeds_out[(size_t)b * max_seeds + k] = sd[k];
        if (hyp_counts_out) hyp_counts_out[(size_t)b * max_seeds + k] = hc[k];
    }
    if (tid != 0) return;
    double* To = T_out + 16 * (size_t)b;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) To[4 * r + c] = T[3 * r + c];
        To[4 * r + 3] = T[9 + r];
    }
    To[12] = 0.0; To[13] = 0.0; To[14] = 0.0; To[15] = 1.0;
    int* io = info + 6 * (size_t)b;
    io[0] = ok ? BUF_SC2_OK : BUF_SC2_NOTHING;
    io[1] = n_live;
    io[2] = n_seeds;
    io[3] = win >= 0 ? sd[win] : -1;
    io[4] = win_count;
    io[5] = (int)fin[0];
}

// ------------------------------------------------------------------------------------------
struct Sc2Ws { int* meta; double* rows; int* live; double* v0; double* v1; double* c; unsigned long long* bits; int* counts; int* seeds;
               int* hypc; double* hypT; };

// rows of C and seed ranks the pairs need: false when a length is out of range
static bool sc2_sizes(const int* corr_lengths, int npairs, int max_seeds, long long& rows, long long& words, long long& counts)
{
    rows = words = counts = 0;
    for (int b = 0; b < npairs; b++) {
        const long long n = corr_lengths[b];
        if (n < 0 || n > BUF_SC2_MAX_ROWS) return false;
        rows += n;
        words += n * ((n + 63) / 64);
        counts += n * (n < max_seeds ? (n > 1 ? n : 1) : max_seeds);     // (seed_ratio <= 1: at most max(1, n) seeds)
    }
    return true;
}

static Sc2Ws carve_sc2(WsCarver& w, int npairs, int max_seeds, long long rows, long long words, long long counts)
{
    Sc2Ws e;
    e.meta = w.take<int>((size_t)npairs * SC2_PAIR_INTS);
    e.rows = w.take<double>(6 * (size_t)rows);
    e.live = w.take<int>((size_t)rows);
    e.v0 = w.take<double>((size_t)rows);
    e.v1 = w.take<double>((size_t)rows);
    e.c = w.take<double>((size_t)rows);
    e.bits = w.take<unsigned long long>((size_t)words);
    e.counts = w.take<int>((size_t)counts);
    e.seeds = w.take<int>((size_t)npairs * max_seeds);
    e.hypc = w.take<int>((size_t)npairs * max_seeds);
    e.hypT = w.take<double>((size_t)npairs * max_seeds * 12);
    return e;
}

extern "C" size_t buf_sc2_ws_bytes(const int* corr_lengths_host, int npairs, int max_seeds)
{
    if (!corr_lengths_host || npairs <= 0 || npairs > SC2_MAX_PAIRS || max_seeds < 1 || max_seeds > SC2_MAX_SEEDS) return 0;
    long long rows, words, counts;
    if (!sc2_sizes(corr_lengths_host, npairs, max_seeds, rows, words, counts)) return 0;
    WsCarver w(nullptr, 0);
    carve_sc2(w, npairs, max_seeds, rows, words, counts);
    return w.used();
}

extern "C" int buf_sc2_batched(const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                               const int* corr, const int* corr_lengths_host, int npairs, double d_thr, double inlier_thr,
                               double seed_ratio, int max_seeds, int k1, double nms_radius, int power_iterations, int refine_iterations,
                               double* T_out, int* info_out, double* conf_out, int* seeds_out, int* hyp_counts_out, int* counts_out,
                               unsigned char* inliers_out, void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const double big = 1.7976931348623157e308;
    BUF_REQUIRE(npairs >= 0 && npairs <= SC2_MAX_PAIRS, BUF_EINVAL, "buf_sc2_batched: npairs=%d (0..%d)", npairs, SC2_MAX_PAIRS);
    BUF_REQUIRE(d_thr > 0.0 && d_thr <= big && d_thr * d_thr > 0.0 && d_thr * d_thr <= big, BUF_EINVAL,
                "buf_sc2_batched: d_thr=%g (must be finite and > 0, and so its square)", d_thr);
    BUF_REQUIRE(inlier_thr > 0.0 && inlier_thr <= big, BUF_EINVAL, "buf_sc2_batched: inlier_thr=%g (must be finite and > 0)", inlier_thr);
    BUF_REQUIRE(seed_ratio > 0.0 && seed_ratio <= 1.0, BUF_EINVAL, "buf_sc2_batched: seed_ratio=%g (must be in (0, 1])", seed_ratio);
    BUF_REQUIRE(max_seeds >= 1 && max_seeds <= SC2_MAX_SEEDS, BUF_EINVAL, "buf_sc2_batched: max_seeds=%d (1..%d)", max_seeds, SC2_MAX_SEEDS);
    BUF_REQUIRE(k1 >= 3 && k1 <= SC2_MAX_K1, BUF_EINVAL, "buf_sc2_batched: k1=%d (3..%d)", k1, SC2_MAX_K1);
    BUF_REQUIRE(nms_radius >= 0.0 && nms_radius <= big, BUF_EINVAL, "buf_sc2_batched: nms_radius=%g (must be finite and >= 0)", nms_radius);
    BUF_REQUIRE(power_iterations >= 0 && power_iterations <= 1000 && refine_iterations >= 0, BUF_EINVAL,
                "buf_sc2_batched: power_iterations=%d (0..1000) refine_iterations=%d", power_iterations, refine_iterations);
    if (npairs == 0) return BUF_OK;
    long long nct, maxn, maxS = 1;
    const int brc = corr_batch_check("buf_sc2_batched", src, src_lengths_host, tgt, tgt_lengths_host, corr, corr_lengths_host, npairs, true,
                                     T_out, info_out, nct, maxn, [&](int b) {
        BUF_REQUIRE(corr_lengths_host[b] <= BUF_SC2_MAX_ROWS, BUF_EINVAL, "buf_sc2_batched: %d correspondences in pair %d (at most %d)",
                    corr_lengths_host[b], b, BUF_SC2_MAX_ROWS);
        return (int)BUF_OK;
    });
    if (brc) return brc;
    long long rows, words, counts;
    sc2_sizes(corr_lengths_host, npairs, max_seeds, rows, words, counts);
    const size_t need = buf_sc2_ws_bytes(corr_lengths_host, npairs, max_seeds);
    BUF_REQUIRE(ws && ws_bytes >= need, BUF_EINVAL, "buf_sc2_batched: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);

    WsCarver w(ws, ws_bytes);
    const Sc2Ws e = carve_sc2(w, npairs, max_seeds, rows, words, counts);
    Sc2Pair* meta = (Sc2Pair*)malloc(sizeof(Sc2Pair) * (size_t)npairs);
    BUF_REQUIRE(meta, BUF_EINVAL, "buf_sc2_batched: out of host memory");
    long long so = 0, to = 0, co = 0, bo = 0, ko = 0;
    for (int b = 0; b < npairs; b++) {
        const long long n = corr_lengths_host[b];
        const double want = ceil(seed_ratio * (double)n);        // S = min(max_seeds, max(1, ceil(seed_ratio n)))
        const int S = want < 1.0 ? 1 : (want > (double)max_seeds ? max_seeds : (int)want);
        Sc2Pair& m = meta[b];
        m.src_off = (int)so; m.ns = src_lengths_host[b]; m.tgt_off = (int)to; m.nt = tgt_lengths_host[b];
        m.corr_off = (int)co; m.n = (int)n; m.S = S; m.pad = 0; m.bits_off = bo; m.cnt_off = ko;
        so += m.ns; to += m.nt; co += n; bo += n * ((n + 63) / 64);
        ko += n * (n < max_seeds ? (n > 1 ? n : 1) : max_seeds);
        maxS = S > maxS ? S : maxS;
    }
    const int rc = upload_ints(e.meta, (const int*)meta, (long long)npairs * SC2_PAIR_INTS, "buf_sc2_batched", s);
    free(meta);
    if (rc) return rc;
    const Sc2Pair* mp = (const Sc2Pair*)e.meta;
    const double d2 = d_thr * d_thr;
    const unsigned int tiles = (unsigned int)(maxn > 0 ? cdiv(maxn, WAVE) : 1), maxW = tiles;
    double pairs2 = 0.0, streamed = 0.0;                         // (work figures of the timing registry)
    for (int b = 0; b < npairs; b++) {
        const double n = corr_lengths_host[b];
        pairs2 += n * n;
        streamed += 8.0 * cdiv(maxS, SC2_SG) * n * (double)((corr_lengths_host[b] + 63) / 64);
    }
    TimedSpan span;
    bool timed = timing_begin(s, &span, pairs2, BUF_TIMED_SC2_COMPAT);
    k_sc2_gather<<<dim3((unsigned int)(maxn > 0 ? cdiv(maxn, SC2_W) : 1), npairs), SC2_W, 0, s>>>(src, tgt, corr, mp, max_seeds, e.rows,
                                                                                                e.live, e.seeds, e.hypc);
    k_sc2_compat<<<dim3((unsigned int)cdiv(maxW, SC2_WAVES), tiles, npairs), SC2_W, 0, s>>>(mp, e.rows, e.live, d_thr, e.bits);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, pairs2 * power_iterations, BUF_TIMED_SC2_CONF);
    const double* v = nullptr;                                   // (nullptr: the start vector of ones)
    for (int it = 0; it < power_iterations; it++) {
        double* vo = (it & 1) ? e.v1 : e.v0;
        k_sc2_power<<<dim3(tiles, npairs), SC2_W, 0, s>>>(mp, e.rows, e.live, e.bits, d2, v, vo);
        v = vo;
    }
    k_sc2_conf<<<dim3(tiles, npairs), WAVE, 0, s>>>(mp, e.rows, e.live, v, nms_radius, e.c, conf_out);
    k_sc2_seeds<<<dim3(tiles, npairs), WAVE, 0, s>>>(mp, e.c, max_seeds, e.seeds);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, streamed, BUF_TIMED_SC2_COUNTS);
    if (counts_out && nct > 0) {
        const long long total = (long long)max_seeds * nct;
        const long long blocks = (total + SC2_W - 1) / SC2_W;
        k_sc2_fill<<<(unsigned int)(blocks < 65536 ? blocks : 65536), SC2_W, 0, s>>>(counts_out, total, -1);
    }
    k_sc2_counts<<<dim3((unsigned int)(maxn > 0 ? cdiv(maxn, SC2_W) : 1), (unsigned int)cdiv(maxS, SC2_SG), npairs), SC2_W, 0, s>>>(
        mp, e.bits, e.seeds, max_seeds, e.counts, counts_out);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, (double)maxS * npairs, BUF_TIMED_SC2_HYP);
    k_sc2_hyp<<<dim3((unsigned int)maxS, npairs), WAVE, 0, s>>>(mp, e.rows, e.live, e.seeds, max_seeds, e.counts, counts_out, k1, d2,
                                                              power_iterations, inlier_thr, e.hypc, e.hypT);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, (double)npairs, BUF_TIMED_SC2_REFINE);
    k_sc2_refine<<<npairs, SC2_W, 0, s>>>(mp, e.rows, e.live, e.seeds, max_seeds, e.hypc, e.hypT, inlier_thr, refine_iterations, T_out,
                                          info_out, seeds_out, hyp_counts_out, inliers_out);
    if (timed) timing_end(s, &span);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
