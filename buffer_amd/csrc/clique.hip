// N10  Max-clique + truncated-least-squares pose estimation on given correspondences, the method made known by TEASER++ (Yang, Shi,
// Carlone, T-RO 2021), restated from its published form with the deviations of include/buffer_hip.h (scale 1, a greedy clique with
// the k-core bound beside it, no certification, N8's refit appended).  B pairs per call, 9 kernels, nothing read back.  The rows,
// the bit matrix, the refit loop and the residual are N8's (sc2.hip), the Kabsch solver and the fixed-shape sums pose_math.h's.
//
//   k_sc2_gather, k_sc2_compat   N8's: rows and the bit matrix C of e_ij <= d_thr (its diagonal bit is masked where the graph is read)
//   k_clique_deg      one wavefront per row: population count of its words, minus the diagonal
//   k_clique_peel     one workgroup of 1024 per pair: degrees, the alive set and the frontier as LDS words.  Level k: the frontier is
//                     the alive rows of degree <= k (core k); they leave the alive set, then each wavefront walks the frontier rows
//                     dealt to it and decrements the alive neighbours with integer LDS atomics (work ~ edges).  An empty frontier
//                     lifts k to the smallest alive degree.  Core numbers are unique: the order of the decrements does not matter.
//   k_clique_order    lane = row: its place by (core desc, deg desc, row asc) by counting; the rows gathered in that order
//   k_sc2_compat      a second time on the gathered rows: in this matrix the first set bit of a word IS the candidate of lowest rank
//   k_clique_walk     one wavefront per seed: the candidate set as up to 4 words per lane; per member a find-first-set in every lane,
//                     a wavefront minimum over the lanes' lowest candidates and one coalesced row load (a chain of dependent L2
//                     loads: latency-bound by construction).  (A ballot + one cross-lane read of the owning word is two shuffles
//                     shorter per member, but returned walks one member too long now and then in large batches: see DESIGN.md.)
//   k_clique_pose     one workgroup per pair: the winner, its members' points in LDS, GNC-TLS over the TIMs (recomputed, never
//                     stored: a weight is a function of the previous rotation and mu), then the three votes (bitonic sort of the 2K
//                     endpoints, a lane per candidate)
//   k_clique_polish   N8's refinement started from that pose (sc2_refit), with its own info words and its own NOTHING rule
// All fp64 without FMA; integer LDS atomics only; every float sum in a fixed shape: a pair's outputs are the same bits alone, in any
// batch and across runs.
#include "pose_math.h"

#define CLQ_PEEL_W 1024
#define CLQ_MAX_SEEDS 1024
#define CLQ_MAX_MEMBERS 512
#define CLQ_PINFO 4                                              // per pair in the workspace: live rows, bound

// grid (rows / 4, pairs): deg = popcount(row) - the diagonal bit; -1 on a dead row
__global__ void __launch_bounds__(SC2_W) k_clique_deg(const Sc2Pair* __restrict__ mp, const int* __restrict__ live,
                                                    const unsigned long long* __restrict__ bits, int* __restrict__ deg)
{
    const Sc2Pair P = mp[blockIdx.y];
    const int n = P.n, W = (n + 63) >> 6, i = blockIdx.x * SC2_WAVES + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (i >= n) return;                                          // (wavefront-uniform)
    const unsigned long long* row = bits + P.bits_off + (long long)i * W;
    int c = 0;
    for (int w = lane; w < W; w += WAVE) c += __popcll(row[w]);
    c = wave_sum(c);
    if (lane == 0) deg[(size_t)P.corr_off + i] = live[(size_t)P.corr_off + i] ? c - 1 : -1;
}

// one workgroup per pair; dynamic LDS: alive u64[W] | front u64[W] | d int[64 W] | frontier size, smallest alive degree, live rows
__global__ void __launch_bounds__(CLQ_PEEL_W) k_clique_peel(const Sc2Pair* __restrict__ mp, const int* __restrict__ live,
                                                          const unsigned long long* __restrict__ bits, const int* __restrict__ deg,
                                                          int* __restrict__ core, int* __restrict__ pinfo)
{
    extern __shared__ unsigned long long clq_lds[];
    const Sc2Pair P = mp[blockIdx.x];
    const int n = P.n, W = (n + 63) >> 6, n64 = W << 6, tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    unsigned long long* alive = clq_lds;
    unsigned long long* front = clq_lds + W;
    int* d = (int*)(clq_lds + 2 * W);
    int* cnt = d + n64;                                          // cnt[0] frontier size, cnt[1] smallest alive degree, cnt[2] live rows
    const unsigned long long* B = bits + P.bits_off;
    if (tid < 3) cnt[tid] = tid == 1 ? 0x7fffffff : 0;
    __syncthreads();
    for (int base = 0; base < n64; base += CLQ_PEEL_W) {
        const int i = base + tid;
        const bool in = i < n, al = in && live[(size_t)P.corr_off + (in ? i : 0)] != 0;
        if (i < n64) d[i] = al ? deg[(size_t)P.corr_off + i] : 0;
        if (in && !al) core[(size_t)P.corr_off + i] = -1;
        const unsigned long long m = __ballot(al);
        if (lane == 0 && i < n64) { alive[i >> 6] = m; atomicAdd(&cnt[2], __popcll(m)); }
    }
    __syncthreads();
    const int n_live = cnt[2];
    int remaining = n_live, k = 0;
    while (remaining > 0) {                                      // (block-uniform: every thread reads the same counters)
        for (int base = 0; base < n64; base += CLQ_PEEL_W) {
            const int i = base + tid;
            const bool al = i < n64 && ((alive[i >> 6] >> (i & 63)) & 1ull);
            const int dv = al ? d[i] : 0x7fffffff;
            const bool f = al && dv <= k;
            if (f) core[(size_t)P.corr_off + i] = k;
            const unsigned long long m = __ballot(f);
            int mn = dv;
            for (int s = WAVE / 2; s > 0; s >>= 1) mn = min(mn, __shfl_xor(mn, s, WAVE));
            if (lane == 0 && i < n64) {
                front[i >> 6] = m;
                if (m) atomicAdd(&cnt[0], __popcll(m));
                if (mn != 0x7fffffff) atomicMin(&cnt[1], mn);
            }
        }
        __syncthreads();
        const int nf = cnt[0], mind = cnt[1];
        if (tid < W) alive[tid] &= ~front[tid];                  // (W <= 256 < the workgroup)
        __syncthreads();
        if (tid == 0) { cnt[0] = 0; cnt[1] = 0x7fffffff; }
        if (nf == 0) {                                           // nothing at this level: on to the smallest alive degree
            if (mind == 0x7fffffff) break;                       // (cannot happen while rows remain; never spin on it)
            k = mind;
            __syncthreads();                                     // the counters are reset before the next pass adds to them
            continue;
        }
        remaining -= nf;
        if (remaining > 0)
            for (int fw = wave; fw < W; fw += CLQ_PEEL_W / WAVE) {   // the frontier rows of word fw belong to this wavefront
                unsigned long long fm = front[fw];
                while (fm) {
                    const int v = (fw << 6) + (__ffsll((long long)fm) - 1);
                    fm &= fm - 1ull;
                    const unsigned long long* row = B + (long long)v * W;
                    for (int w = lane; w < W; w += WAVE) {
                        unsigned long long m = row[w] & alive[w];
                        while (m) {
                            atomicSub(&d[(w << 6) + (__ffsll((long long)m) - 1)], 1);
                            m &= m - 1ull;
                        }
                    }
                }
            }
        __syncthreads();
    }
    if (tid == 0) {
        pinfo[CLQ_PINFO * blockIdx.x] = n_live;
        pinfo[CLQ_PINFO * blockIdx.x + 1] = n_live > 0 ? k + 1 : 0;
    }
}

// grid (row tiles of 256, pairs): rank by counting, the rows gathered in rank order (dead rows behind the live ones, as zeros)
__global__ void __launch_bounds__(SC2_W) k_clique_order(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                      const int* __restrict__ deg, const int* __restrict__ core,
                                                      const int* __restrict__ pinfo, int* __restrict__ order, double* __restrict__ rows2,
                                                      int* __restrict__ live2, int* __restrict__ deg_out, int* __restrict__ core_out,
                                                      int* __restrict__ rank_out)
{
    const Sc2Pair P = mp[blockIdx.y];
    const int n = P.n, i = blockIdx.x * SC2_W + threadIdx.x;
    if (i >= n) return;
    const int* dg = deg + P.corr_off, *cr = core + P.corr_off;
    const int di = dg[i], ci = cr[i];
    const bool li = di >= 0;
    int place = 0;
    if (li) {
        for (int j = 0; j < n; j++) {
            const int cj = cr[j], dj = dg[j];
            place += (cj > ci || (cj == ci && (dj > di || (dj == di && j < i)))) ? 1 : 0;
        }
    } else {
        place = pinfo[CLQ_PINFO * blockIdx.y];
        for (int j = 0; j < i; j++) place += dg[j] < 0 ? 1 : 0;
    }
    const size_t g = (size_t)P.corr_off + i, g2 = (size_t)P.corr_off + place;
    order[g2] = i;
    live2[g2] = li ? 1 : 0;
    for (int c = 0; c < 6; c++) rows2[6 * g2 + c] = li ? rows[6 * g + c] : 0.0;
    if (deg_out) deg_out[g] = di;
    if (core_out) core_out[g] = ci;
    if (rank_out) rank_out[g] = li ? place : -1;
}

// grid (seed ranks, pairs), one wavefront per seed, in rank space (bits2): sizes[rank] = the walk's length, its first max_members
// members into walks
__global__ void __launch_bounds__(WAVE) k_clique_walk(const Sc2Pair* __restrict__ mp, const unsigned long long* __restrict__ bits2,
                                                    const int* __restrict__ pinfo, int max_seeds, int max_members,
                                                    int* __restrict__ sizes, int* __restrict__ walks)
{
    const Sc2Pair P = mp[blockIdx.y];
    const int n = P.n, W = (n + 63) >> 6, r = blockIdx.x, lane = threadIdx.x;
    if (r >= pinfo[CLQ_PINFO * blockIdx.y]) return;              // (fewer live rows than seed ranks: sizes holds -1 from k_sc2_gather)
    const unsigned long long* B = bits2 + P.bits_off;
    int* walk = walks + ((size_t)blockIdx.y * max_seeds + r) * max_members;
    const unsigned long long* row = B + (long long)r * W;
    unsigned long long c0 = lane < W ? row[lane] : 0ull, c1 = lane + 64 < W ? row[lane + 64] : 0ull;
    unsigned long long c2 = lane + 128 < W ? row[lane + 128] : 0ull, c3 = lane + 192 < W ? row[lane + 192] : 0ull;
    {                                                            // the seed's own bit
        const unsigned long long keep = ~(1ull << (r & 63));
        const int w = r >> 6;
        if (lane == (w & 63)) { if (w < 64) c0 &= keep; else if (w < 128) c1 &= keep; else if (w < 192) c2 &= keep; else c3 &= keep; }
    }
    if (lane == 0) walk[0] = r;
    int len = 1;
    for (;;) {
        int j = 0x7fffffff;                                      // the lowest candidate of this lane's words, then of the wavefront
        if (c0) j = (lane << 6) + (__ffsll((long long)c0) - 1);
        else if (c1) j = ((lane + 64) << 6) + (__ffsll((long long)c1) - 1);
        else if (c2) j = ((lane + 128) << 6) + (__ffsll((long long)c2) - 1);
        else if (c3) j = ((lane + 192) << 6) + (__ffsll((long long)c3) - 1);
        for (int d = WAVE / 2; d > 0; d >>= 1) j = min(j, __shfl_xor(j, d, WAVE));
        if (j == 0x7fffffff) break;                              // (j < n: bits past n are never set)
        const int h = j >> 12, sl = (j >> 6) & 63;
        row = B + (long long)j * W;
        c0 &= lane < W ? row[lane] : 0ull;
        if (W > 64) {
            c1 &= lane + 64 < W ? row[lane + 64] : 0ull;
            c2 &= lane + 128 < W ? row[lane + 128] : 0ull;
            c3 &= lane + 192 < W ? row[lane + 192] : 0ull;
        }
        if (lane == sl) {                                        // row j carries its own diagonal bit
            const unsigned long long keep = ~(1ull << (j & 63));
            if (h == 0) c0 &= keep; else if (h == 1) c1 &= keep; else if (h == 2) c2 &= keep; else c3 &= keep;
        }
        if (lane == 0 && len < max_members) walk[len] = j;
        len++;
    }
    if (lane == 0) sizes[(size_t)blockIdx.y * max_seeds + r] = len;
}

// the TLS weight of a squared residual under (mu, c2)
__device__ __forceinline__ double clq_weight(double r2, double mu, double c2, double hi, double lo)
{
    if (r2 >= hi) return 0.0;
    if (r2 <= lo) return 1.0;
    return sqrt((c2 * (mu * (mu + 1.0))) / r2) - mu;
}

// |beta - R alpha|^2 of the TIM (a, b) of the members' rows sr
__device__ __forceinline__ double clq_tim_r2(const double* R, const double* ra, const double* rb, double* al, double* be)
{
    for (int c = 0; c < 3; c++) { al[c] = rb[c] - ra[c]; be[c] = rb[3 + c] - ra[3 + c]; }
    const double x = be[0] - ((R[0] * al[0] + R[1] * al[1]) + R[2] * al[2]);
    const double y = be[1] - ((R[3] * al[0] + R[4] * al[1]) + R[5] * al[2]);
    const double z = be[2] - ((R[6] * al[0] + R[7] * al[1]) + R[8] * al[2]);
    return (x * x + y * y) + z * z;
}

__device__ __forceinline__ double clq_block_max(double v, double* red)
{
    v = sc2_wave_max(v);
    __syncthreads();
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// one workgroup per pair: winner, members, GNC-TLS rotation, voted translation -> pose0 and the first seven info words (workspace)
__global__ void __launch_bounds__(SC2_W) k_clique_pose(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                     const int* __restrict__ order, const int* __restrict__ pinfo,
                                                     const int* __restrict__ sizes, const int* __restrict__ walks, int max_seeds,
                                                     int max_members, double c2, double t_thr, double gnc_factor, int gnc_iterations,
                                                     double* __restrict__ pose0, int* __restrict__ ginfo, int* __restrict__ sizes_out,
                                                     int* __restrict__ members_out, double* __restrict__ weights_out,
                                                     double* __restrict__ pose0_out)
{
    __shared__ double sr[CLQ_MAX_MEMBERS][6];
    __shared__ double ep[2 * CLQ_MAX_MEMBERS];
    __shared__ double xs[CLQ_MAX_MEMBERS];
    __shared__ double red[SC2_WAVES * 9];
    __shared__ unsigned long long wbest[SC2_WAVES];
    __shared__ double bcost[SC2_WAVES], best_est[SC2_WAVES];
    __shared__ int bj[SC2_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const Sc2Pair P = mp[b];
    const int n_live = pinfo[CLQ_PINFO * b], bound = pinfo[CLQ_PINFO * b + 1];
    const int S = n_live < max_seeds ? n_live : max_seeds;
    const int* sz = sizes + (size_t)b * max_seeds;

    unsigned long long best = 0ull;                              // the largest size, ties to the lowest rank
    for (int r = tid; r < S; r += SC2_W) {
        const unsigned long long key = ((unsigned long long)(unsigned int)sz[r] << 32) | (unsigned long long)(0xffffffffu - (unsigned int)r);
        best = key > best ? key : best;
    }
    best = sc2_wave_max_u64(best);
    if (lane == 0) wbest[wave] = best;
    __syncthreads();
    best = 0ull;
    for (int w = 0; w < SC2_WAVES; w++) best = wbest[w] > best ? wbest[w] : best;
    const int win = best ? (int)(0xffffffffu - (unsigned int)(best & 0xffffffffull)) : -1;
    const int size = best ? (int)(best >> 32) : 0;
    const int K = size < max_members ? size : max_members;
    const int* walk = walks + ((size_t)b * max_seeds + (win >= 0 ? win : 0)) * max_members;
    for (int k = tid; k < max_members; k += SC2_W) {
        const int row = k < K ? order[(size_t)P.corr_off + walk[k]] : -1;
        if (members_out) members_out[(size_t)b * max_members + k] = row;
        if (k < K)
            for (int c = 0; c < 6; c++) sr[k][c] = rows[6 * ((size_t)P.corr_off + row) + c];
    }
    if (sizes_out)
        for (int k = tid; k < max_seeds; k += SC2_W) sizes_out[(size_t)b * max_seeds + k] = k < S ? sz[k] : -1;
    const long long Mmax = (long long)max_members * (max_members - 1) / 2;
    double* wo = weights_out ? weights_out + (size_t)b * Mmax : nullptr;
    const long long M = (long long)K * (K - 1) / 2;
    if (wo)
        for (long long k = (size < 3 ? 0 : M) + tid; k < Mmax; k += SC2_W) wo[k] = __builtin_nan("");
    __syncthreads();

    double R[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 }, t[3] = { 0.0, 0.0, 0.0 };
    int steps = 0;
    if (size >= 3) {                                             // (block-uniform)
        // ---- GNC-TLS over the TIMs: thread tid takes the TIMs (a, a + 1 + tid + 256 k) of every a
        double mu = 0.0, mu_prev = 0.0, Rp[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
        double pz = 0.0, po = (double)M;
        bool all_one = false;
        for (int it = 0; it < gnc_iterations; it++) {
            steps = it + 1;
            const double hi_p = it > 0 ? ((mu_prev + 1.0) / mu_prev) * c2 : 0.0, lo_p = it > 0 ? (mu_prev / (mu_prev + 1.0)) * c2 : 0.0;
            double H[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, al[3], be[3];
            for (int a = 0; a < K - 1; a++)
                for (int bb = a + 1 + tid; bb < K; bb += SC2_W) {
                    const double r2 = clq_tim_r2(Rp, sr[a], sr[bb], al, be);
                    const double w = it > 0 ? clq_weight(r2, mu_prev, c2, hi_p, lo_p) : 1.0;
                    for (int r = 0; r < 3; r++)
                        for (int c = 0; c < 3; c++) H[3 * r + c] += (w * al[r]) * be[c];
                }
            tile_sum<9, SC2_WAVES>(H, red);
            for (int k = 0; k < 9; k++) R[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
            if (finite9(H)) kabsch_rotation(H, R);
            if (it == 0) {
                double mx = 0.0;
                for (int a = 0; a < K - 1; a++)
                    for (int bb = a + 1 + tid; bb < K; bb += SC2_W) mx = fmax(mx, clq_tim_r2(R, sr[a], sr[bb], al, be));
                mx = clq_block_max(mx, red);
                const double g = (2.0 * mx) / c2 - 1.0;
                if (g <= 0.0) { all_one = true; break; }
                mu = 1.0 / g;
            }
            const double hi = ((mu + 1.0) / mu) * c2, lo = (mu / (mu + 1.0)) * c2;
            double zo[2] = { 0.0, 0.0 };                         // (counts below 2^53: exact in fp64)
            for (int a = 0; a < K - 1; a++)
                for (int bb = a + 1 + tid; bb < K; bb += SC2_W) {
                    const double w = clq_weight(clq_tim_r2(R, sr[a], sr[bb], al, be), mu, c2, hi, lo);
                    zo[0] += w == 0.0 ? 1.0 : 0.0;
                    zo[1] += w == 1.0 ? 1.0 : 0.0;
                }
            tile_sum<2, SC2_WAVES>(zo, red);
            for (int k = 0; k < 9; k++) Rp[k] = R[k];
            mu_prev = mu;
            if ((it >= 1 && zo[0] + zo[1] == (double)M && zo[0] == pz && zo[1] == po) || it + 1 == gnc_iterations) break;
            pz = zo[0]; po = zo[1];
            mu = mu * gnc_factor;
        }
        if (wo) {
            const double hi = all_one ? 0.0 : ((mu_prev + 1.0) / mu_prev) * c2, lo = all_one ? 0.0 : (mu_prev / (mu_prev + 1.0)) * c2;
            double al[3], be[3];
            for (int a = 0; a < K - 1; a++) {
                const long long base = (long long)a * K - (long long)a * (a + 1) / 2 - (a + 1);
                for (int bb = a + 1 + tid; bb < K; bb += SC2_W)
                    wo[base + bb] = all_one ? 1.0 : clq_weight(clq_tim_r2(R, sr[a], sr[bb], al, be), mu_prev, c2, hi, lo);
            }
        }
        // ---- the three votes
        const int E = 2 * K;
        int N2 = 2;
        while (N2 < E) N2 <<= 1;
        const double cc = t_thr * t_thr;
        for (int ax = 0; ax < 3; ax++) {
            __syncthreads();
            for (int k = tid; k < K; k += SC2_W) {
                const double v = sr[k][3 + ax] - ((R[3 * ax] * sr[k][0] + R[3 * ax + 1] * sr[k][1]) + R[3 * ax + 2] * sr[k][2]);
                xs[k] = v;
                ep[2 * k] = v - t_thr;
                ep[2 * k + 1] = v + t_thr;
            }
            for (int k = E + tid; k < N2; k += SC2_W) ep[k] = __builtin_inf();
            __syncthreads();
            for (int kk = 2; kk <= N2; kk <<= 1)
                for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                    for (int i = tid; i < N2; i += SC2_W) {
                        const int l = i ^ jj;
                        if (l > i) {
                            const double x = ep[i], y = ep[l];
                            if (((i & kk) == 0) ? (x > y) : (x < y)) { ep[i] = y; ep[l] = x; }
                        }
                    }
                    __syncthreads();
                }
            double mc = __builtin_inf(), me = 0.0;
            int mj = 0x7fffffff;
            for (int j = tid; j < E - 1; j += SC2_W) {
                const double h = (ep[j] + ep[j + 1]) * 0.5;
                double s = 0.0;
                int cnt = 0;
                for (int k = 0; k < K; k++)
                    if (fabs(xs[k] - h) <= t_thr) { s += xs[k]; cnt++; }
                if (cnt == 0) continue;
                const double est = s / (double)cnt;
                double q = 0.0;
                for (int k = 0; k < K; k++)
                    if (fabs(xs[k] - h) <= t_thr) q += (xs[k] - est) * (xs[k] - est);
                const double cost = q + (double)(K - cnt) * cc;
                if (cost < mc) { mc = cost; me = est; mj = j; }  // (ascending j per thread: ties keep the lowest)
            }
            for (int d = WAVE / 2; d > 0; d >>= 1) {
                const double oc = __shfl_xor(mc, d, WAVE), oe = __shfl_xor(me, d, WAVE);
                const int oj = __shfl_xor(mj, d, WAVE);
                if (oc < mc || (oc == mc && oj < mj)) { mc = oc; me = oe; mj = oj; }
            }
            if (lane == 0) { bcost[wave] = mc; best_est[wave] = me; bj[wave] = mj; }
            __syncthreads();
            mc = bcost[0]; me = best_est[0]; mj = bj[0];
            for (int w = 1; w < SC2_WAVES; w++)
                if (bcost[w] < mc || (bcost[w] == mc && bj[w] < mj)) { mc = bcost[w]; me = best_est[w]; mj = bj[w]; }
            t[ax] = mj == 0x7fffffff ? 0.0 : me;
        }
    }
    if (tid != 0) return;
    for (int k = 0; k < 12; k++) {
        const double v = k < 9 ? R[k] : t[k - 9];
        pose0[12 * (size_t)b + k] = v;
        if (pose0_out) pose0_out[12 * (size_t)b + k] = v;
    }
    int* g = ginfo + 8 * (size_t)b;
    g[0] = size >= 3 ? BUF_CLIQUE_OK : BUF_CLIQUE_NOTHING;
    g[1] = n_live; g[2] = bound; g[3] = size; g[4] = win; g[5] = K; g[6] = steps; g[7] = 0;
}

// one workgroup per pair: N8's refinement from pose0 (sc2_refit), NOTHING below 3 final inliers, every remaining output
__global__ void __launch_bounds__(SC2_W) k_clique_polish(const Sc2Pair* __restrict__ mp, const double* __restrict__ rows,
                                                       const int* __restrict__ live, const double* __restrict__ pose0,
                                                       const int* __restrict__ ginfo, double inlier_thr, int refine_iterations,
                                                       double* __restrict__ T_out, int* __restrict__ info,
                                                       unsigned char* __restrict__ inliers_out)
{
    __shared__ double red[SC2_WAVES * 9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Sc2Pair P = mp[b];
    const int n = P.n;
    const double* R = rows + 6 * (size_t)P.corr_off;
    const int* L = live + P.corr_off;
    const bool ok = ginfo[8 * (size_t)b] == BUF_CLIQUE_OK;
    double T[12];
    for (int k = 0; k < 12; k++) T[k] = pose0[12 * (size_t)b + k];
    if (ok) sc2_refit(R, L, n, inlier_thr, refine_iterations, red, T);
    double fin[1] = { 0.0 };
    for (int i = tid; i < n; i += SC2_W) fin[0] += (ok && L[i] && sc2_residual(T, R + 6 * (size_t)i) < inlier_thr) ? 1.0 : 0.0;
    tile_sum<1, SC2_WAVES>(fin, red);
    const bool good = ok && fin[0] >= 3.0;
    if (inliers_out)
        for (int i = tid; i < n; i += SC2_W)
            inliers_out[(size_t)P.corr_off + i] = (good && L[i] && sc2_residual(T, R + 6 * (size_t)i) < inlier_thr) ? 1 : 0;
    if (tid != 0) return;
    double* To = T_out + 16 * (size_t)b;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) To[4 * r + c] = good ? T[3 * r + c] : (r == c ? 1.0 : 0.0);
        To[4 * r + 3] = good ? T[9 + r] : 0.0;
    }
    To[12] = 0.0; To[13] = 0.0; To[14] = 0.0; To[15] = 1.0;
    int* io = info + 8 * (size_t)b;
    for (int k = 1; k < 7; k++) io[k] = ginfo[8 * (size_t)b + k];
    io[0] = good ? BUF_CLIQUE_OK : BUF_CLIQUE_NOTHING;
    io[7] = good ? (int)fin[0] : 0;
}

// ------------------------------------------------------------------------------------------
struct CliqueWs { int* meta; double* rows; int* live; double* rows2; int* live2; unsigned long long* bits; unsigned long long* bits2;
                  int* deg; int* core; int* order; int* pinfo; int* sizes; int* spare; int* walks; double* pose0; int* ginfo; };

static CliqueWs carve_clique(WsCarver& w, int npairs, int max_seeds, int max_members, long long rows, long long words)
{
    CliqueWs e;
    e.meta = w.take<int>((size_t)npairs * SC2_PAIR_INTS);
    e.rows = w.take<double>(6 * (size_t)rows);
    e.live = w.take<int>((size_t)rows);
    e.rows2 = w.take<double>(6 * (size_t)rows);
    e.live2 = w.take<int>((size_t)rows);
    e.bits = w.take<unsigned long long>((size_t)words);
    e.bits2 = w.take<unsigned long long>((size_t)words);
    e.deg = w.take<int>((size_t)rows);
    e.core = w.take<int>((size_t)rows);
    e.order = w.take<int>((size_t)rows);
    e.pinfo = w.take<int>((size_t)npairs * CLQ_PINFO);
    e.sizes = w.take<int>((size_t)npairs * max_seeds);
    e.spare = w.take<int>((size_t)npairs * max_seeds);
    e.walks = w.take<int>((size_t)npairs * max_seeds * max_members);
    e.pose0 = w.take<double>((size_t)npairs * 12);
    e.ginfo = w.take<int>((size_t)npairs * 8);
    return e;
}

extern "C" size_t buf_clique_ws_bytes(const int* corr_lengths_host, int npairs, int max_seeds, int max_members)
{
    if (!corr_lengths_host || npairs <= 0 || npairs > SC2_MAX_PAIRS || max_seeds < 1 || max_seeds > CLQ_MAX_SEEDS || max_members < 3 ||
        max_members > CLQ_MAX_MEMBERS)
        return 0;
    long long rows, words, counts;
    if (!sc2_sizes(corr_lengths_host, npairs, max_seeds, rows, words, counts)) return 0;
    WsCarver w(nullptr, 0);
    carve_clique(w, npairs, max_seeds, max_members, rows, words);
    return w.used();
}

extern "C" int buf_clique_batched(const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                                  const int* corr, const int* corr_lengths_host, int npairs, double d_thr, double tim_thr, double t_thr,
                                  double inlier_thr, int max_seeds, int max_members, double gnc_factor, int gnc_iterations,
                                  int refine_iterations, double* T_out, int* info_out, int* deg_out, int* core_out, int* rank_out,
                                  int* sizes_out, int* members_out, double* weights_out, double* pose0_out, unsigned char* inliers_out,
                                  void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const double big = 1.7976931348623157e308;
    BUF_REQUIRE(npairs >= 0 && npairs <= SC2_MAX_PAIRS, BUF_EINVAL, "buf_clique_batched: npairs=%d (0..%d)", npairs, SC2_MAX_PAIRS);
    BUF_REQUIRE(d_thr > 0.0 && d_thr <= big, BUF_EINVAL, "buf_clique_batched: d_thr=%g (must be finite and > 0)", d_thr);
    BUF_REQUIRE(tim_thr > 0.0 && tim_thr <= big && tim_thr * tim_thr > 0.0 && tim_thr * tim_thr <= big, BUF_EINVAL,
                "buf_clique_batched: tim_thr=%g (must be finite and > 0, and so its square)", tim_thr);
    BUF_REQUIRE(t_thr > 0.0 && t_thr <= big && t_thr * t_thr > 0.0 && t_thr * t_thr <= big, BUF_EINVAL,
                "buf_clique_batched: t_thr=%g (must be finite and > 0, and so its square)", t_thr);
    BUF_REQUIRE(inlier_thr > 0.0 && inlier_thr <= big, BUF_EINVAL, "buf_clique_batched: inlier_thr=%g (must be finite and > 0)", inlier_thr);
    BUF_REQUIRE(max_seeds >= 1 && max_seeds <= CLQ_MAX_SEEDS, BUF_EINVAL, "buf_clique_batched: max_seeds=%d (1..%d)", max_seeds, CLQ_MAX_SEEDS);
    BUF_REQUIRE(max_members >= 3 && max_members <= CLQ_MAX_MEMBERS, BUF_EINVAL, "buf_clique_batched: max_members=%d (3..%d)", max_members,
                CLQ_MAX_MEMBERS);
    BUF_REQUIRE(gnc_factor > 1.0 && gnc_factor <= big, BUF_EINVAL, "buf_clique_batched: gnc_factor=%g (must be finite and > 1)", gnc_factor);
    BUF_REQUIRE(gnc_iterations >= 1 && gnc_iterations <= 1000 && refine_iterations >= 0, BUF_EINVAL,
                "buf_clique_batched: gnc_iterations=%d (1..1000) refine_iterations=%d", gnc_iterations, refine_iterations);
    if (npairs == 0) return BUF_OK;
    long long nct, maxn;
    const int brc = corr_batch_check("buf_clique_batched", src, src_lengths_host, tgt, tgt_lengths_host, corr, corr_lengths_host, npairs, true,
                                     T_out, info_out, nct, maxn, [&](int b) {
        BUF_REQUIRE(corr_lengths_host[b] <= BUF_SC2_MAX_ROWS, BUF_EINVAL, "buf_clique_batched: %d correspondences in pair %d (at most %d)",
                    corr_lengths_host[b], b, BUF_SC2_MAX_ROWS);
        return (int)BUF_OK;
    });
    if (brc) return brc;
    long long rows, words, counts;
    sc2_sizes(corr_lengths_host, npairs, max_seeds, rows, words, counts);
    const size_t need = buf_clique_ws_bytes(corr_lengths_host, npairs, max_seeds, max_members);
    BUF_REQUIRE(ws && ws_bytes >= need, BUF_EINVAL, "buf_clique_batched: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);

    WsCarver w(ws, ws_bytes);
    const CliqueWs e = carve_clique(w, npairs, max_seeds, max_members, rows, words);
    Sc2Pair* meta = (Sc2Pair*)malloc(sizeof(Sc2Pair) * (size_t)npairs);
    BUF_REQUIRE(meta, BUF_EINVAL, "buf_clique_batched: out of host memory");
    long long so = 0, to = 0, co = 0, bo = 0;
    double pairs2 = 0.0;
    for (int b = 0; b < npairs; b++) {
        const long long n = corr_lengths_host[b];
        Sc2Pair& m = meta[b];
        m.src_off = (int)so; m.ns = src_lengths_host[b]; m.tgt_off = (int)to; m.nt = tgt_lengths_host[b];
        m.corr_off = (int)co; m.n = (int)n; m.S = (int)(n < max_seeds ? n : max_seeds); m.pad = 0; m.bits_off = bo; m.cnt_off = 0;
        so += m.ns; to += m.nt; co += n; bo += n * ((n + 63) / 64);
        pairs2 += (double)n * (double)n;
    }
    const int rc = upload_ints(e.meta, (const int*)meta, (long long)npairs * SC2_PAIR_INTS, "buf_clique_batched", s);
    free(meta);
    if (rc) return rc;
    const Sc2Pair* mp = (const Sc2Pair*)e.meta;
    const unsigned int tiles = (unsigned int)(maxn > 0 ? cdiv(maxn, WAVE) : 1), maxW = tiles;
    const unsigned int tiles256 = (unsigned int)(maxn > 0 ? cdiv(maxn, SC2_W) : 1);
    const unsigned int maxS = (unsigned int)(maxn < max_seeds ? (maxn > 0 ? maxn : 1) : max_seeds);
    const size_t peel_lds = (size_t)maxW * (2 * 8 + 64 * 4) + 16;
    static LdsGrant peel_grant;
    if (int grc = grant_dynamic_lds((const void*)k_clique_peel, peel_lds, peel_grant)) return grc;

    TimedSpan span;
    bool timed = timing_begin(s, &span, pairs2, BUF_TIMED_CLIQUE_GRAPH);
    k_sc2_gather<<<dim3(tiles256, npairs), SC2_W, 0, s>>>(src, tgt, corr, mp, max_seeds, e.rows, e.live, e.sizes, e.spare);
    k_sc2_compat<<<dim3((unsigned int)cdiv(maxW, SC2_WAVES), tiles, npairs), SC2_W, 0, s>>>(mp, e.rows, e.live, d_thr, e.bits);
    k_clique_deg<<<dim3((unsigned int)(maxn > 0 ? cdiv(maxn, SC2_WAVES) : 1), npairs), SC2_W, 0, s>>>(mp, e.live, e.bits, e.deg);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, (double)npairs, BUF_TIMED_CLIQUE_PEEL);
    k_clique_peel<<<npairs, CLQ_PEEL_W, peel_lds, s>>>(mp, e.live, e.bits, e.deg, e.core, e.pinfo);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, 2.0 * pairs2, BUF_TIMED_CLIQUE_ORDER);
    k_clique_order<<<dim3(tiles256, npairs), SC2_W, 0, s>>>(mp, e.rows, e.deg, e.core, e.pinfo, e.order, e.rows2, e.live2, deg_out, core_out,
                                                          rank_out);
    k_sc2_compat<<<dim3((unsigned int)cdiv(maxW, SC2_WAVES), tiles, npairs), SC2_W, 0, s>>>(mp, e.rows2, e.live2, d_thr, e.bits2);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, (double)maxS * npairs, BUF_TIMED_CLIQUE_WALK);
    k_clique_walk<<<dim3(maxS, npairs), WAVE, 0, s>>>(mp, e.bits2, e.pinfo, max_seeds, max_members, e.sizes, e.walks);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, (double)npairs, BUF_TIMED_CLIQUE_POSE);
    k_clique_pose<<<npairs, SC2_W, 0, s>>>(mp, e.rows, e.order, e.pinfo, e.sizes, e.walks, max_seeds, max_members, tim_thr * tim_thr, t_thr,
                                           gnc_factor, gnc_iterations, e.pose0, e.ginfo, sizes_out, members_out, weights_out, pose0_out);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, (double)npairs, BUF_TIMED_CLIQUE_POLISH);
    k_clique_polish<<<npairs, SC2_W, 0, s>>>(mp, e.rows, e.live, e.pose0, e.ginfo, inlier_thr, refine_iterations, T_out, info_out,
                                             inliers_out);
    if (timed) timing_end(s, &span);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
