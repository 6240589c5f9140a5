// N7  Fast Global Registration (Zhou, Park, Koltun 2016; open3d registration_fast_based_on_feature_matching restated from its
// published form, unpinned: the contract is in include/buffer_hip.h), B pairs per call, two launches, nothing read back.
//
//   k_fgr_tuples    one workgroup per pair.  The trials are taken FGR_W at a time in ascending order; a lane draws its three
//                   correspondences (splitmix64, the mixer of registration.hip), forms the six squared edges in fp64 and decides.
//                   The accepted trials of a chunk are compacted in trial order (ballot inside a wavefront, the four wavefront
//                   counts through LDS), so the kept list does not depend on the chunk width; the lane whose trial takes the last
//                   slot records its index.
//   k_fgr_optimize  one workgroup per pair runs normalisation and all Gauss-Newton steps.  Lane k sums rows k, k + FGR_W, ... in
//                   ascending order; the 27 sums of a step go through a xor-shuffle tree inside each wavefront and a fixed tree over
//                   the four wavefronts in LDS; lane 0 solves and updates the pose, which the others read back from LDS.  The
//                   normalised kept points live in the workspace (48 bytes per row), formed once.
// No float atomics and a fixed order in every sum: a pair's outputs are the same bits alone, in any batch and across runs.
#include "common.h"
#include "pose_math.h"

#define FGR_W 256
#define FGR_WAVES (FGR_W / WAVE)
#define FGR_NV 27
#define FGR_MAX_TUPLES 4096
#define FGR_MIN_ROWS 10

__device__ __forceinline__ double fgr_edge2(const double* a, const double* b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the decision of trial t; on acceptance rows[0..5] = (src row, tgt row) of its three correspondences
__device__ __forceinline__ bool fgr_trial(const float* __restrict__ src, int ns, const float* __restrict__ tgt, int nt,
                                          const int* __restrict__ corr, int n, unsigned long long seed, int t, double s2, int rows[6])
{
    double P[3][3], Q[3][3];                                     // source, target
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        const int r = (int)(splitmix64(seed + 3ull * (unsigned long long)t + (unsigned long long)k) % (unsigned long long)n);
        const int is = corr[2 * (size_t)r], it = corr[2 * (size_t)r + 1];
        rows[2 * k] = is; rows[2 * k + 1] = it;
        const bool in = (unsigned int)is < (unsigned int)ns && (unsigned int)it < (unsigned int)nt;
        ok = ok && in;
        for (int c = 0; c < 3; c++) {
            P[k][c] = in ? (double)src[3 * (size_t)is + c] : 0.0;
            Q[k][c] = in ? (double)tgt[3 * (size_t)it + c] : 0.0;
            ok = ok && isfinite(P[k][c]) && isfinite(Q[k][c]);
        }
    }
    for (int e = 0; e < 3; e++) {                                // edges (0,1), (1,2), (2,0)
        const int i = e, j = (e + 1) % 3;
        const double a = fgr_edge2(Q[i], Q[j]), b = fgr_edge2(P[i], P[j]);
        ok = ok && (s2 * a < b) && (s2 * b < a);
    }
    return ok;
}

// meta: [src_off (B + 1) | tgt_off (B + 1) | corr_off (B + 1) | seeds (2 B: low word, high word)]
__global__ void __launch_bounds__(FGR_W) k_fgr_tuples(const float* __restrict__ src, const float* __restrict__ tgt,
                                                    const int* __restrict__ corr, const int* __restrict__ meta, int npairs,
                                                    double s2, int max_tuples, int trial_factor, int* __restrict__ rows_all,
                                                    int* __restrict__ info)
{
    __shared__ int wcnt[FGR_WAVES];
    __shared__ int examined;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int* src_off = meta, *tgt_off = meta + (npairs + 1), *corr_off = meta + 2 * (npairs + 1);
    const unsigned int* sd = (const unsigned int*)(meta + 3 * (npairs + 1));
    const unsigned long long seed = (unsigned long long)sd[2 * b] | ((unsigned long long)sd[2 * b + 1] << 32);
    const int ns = src_off[b + 1] - src_off[b], nt = tgt_off[b + 1] - tgt_off[b], n = corr_off[b + 1] - corr_off[b];
    const float* S = src + 3 * (size_t)src_off[b], *T = tgt + 3 * (size_t)tgt_off[b];
    const int* Cr = corr + 2 * (size_t)corr_off[b];
    int* rows = rows_all + (size_t)b * 6 * max_tuples;
    const int ntrial = trial_factor * n;                         // (the host checked the product)
    if (tid == 0) examined = ntrial;
    int kept = 0;
    for (int c0 = 0; c0 < ntrial && kept < max_tuples; c0 += FGR_W) {       // (block-uniform: kept is the same in every lane)
        const int t = c0 + tid;
        int r[6];
        const bool acc = t < ntrial && fgr_trial(S, ns, T, nt, Cr, n, seed, t, s2, r);
        const unsigned long long m = __ballot(acc);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int base = kept, total = 0;
#pragma unroll
        for (int w = 0; w < FGR_WAVES; w++) {
            if (w < wave) base += wcnt[w];
            total += wcnt[w];
        }
        const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
        if (acc && slot < max_tuples) {
#pragma unroll
            for (int k = 0; k < 6; k++) rows[6 * (size_t)slot + k] = r[k];
            if (slot == max_tuples - 1) examined = t + 1;
        }
        kept = kept + total < max_tuples ? kept + total : max_tuples;
        __syncthreads();
    }
    __syncthreads();
    for (int i = 6 * kept + tid; i < 6 * max_tuples; i += FGR_W) rows[i] = -1;
    if (tid == 0) {
        info[4 * b + 1] = kept;
        info[4 * b + 2] = examined;
    }
}

// ------------------------------------------------------------------------------------------
// mean of the finite rows of a cloud -> c[3] in thread 0 (count in cnt); lane k adds rows k, k + FGR_W, ...
__device__ __forceinline__ void fgr_mean(const float* __restrict__ p, int n, double* red, double c[3], double& cnt)
{
    double v[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < n; i += FGR_W) {
        const double x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) { v[0] += x; v[1] += y; v[2] += z; v[3] += 1.0; }
    }
    tile_sum<4, FGR_WAVES, false>(v, red);
    cnt = v[3];
    for (int k = 0; k < 3; k++) c[k] = v[k] / v[3];
}

// largest centred squared norm of the finite rows, in every lane's own share (the maximum over lanes is taken by the caller)
__device__ __forceinline__ double fgr_max_norm2(const float* __restrict__ p, int n, const double* c)
{
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += FGR_W) {
        const double x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            const double dx = x - c[0], dy = y - c[1], dz = z - c[2];
            m = fmax(m, (dx * dx + dy * dy) + dz * dz);
        }
    }
    return m;
}

// T <- dT(x) T on T = [R (9, row-major) | t (3)], dT = [Rz(x2) Ry(x1) Rx(x0) | x3..5]
__device__ static void fgr_apply(const double (&x)[6], double* T)
{
    double d[9], n[12];
    rot_zyx(x, d);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) n[3 * r + c] = (d[3 * r] * T[c] + d[3 * r + 1] * T[3 + c]) + d[3 * r + 2] * T[6 + c];
        n[9 + r] = ((d[3 * r] * T[9] + d[3 * r + 1] * T[10]) + d[3 * r + 2] * T[11]) + x[3 + r];
    }
    for (int k = 0; k < 12; k++) T[k] = n[k];
}

__global__ void __launch_bounds__(FGR_W) k_fgr_optimize(const float* __restrict__ src, const float* __restrict__ tgt,
                                                      const int* __restrict__ meta, int npairs, const int* __restrict__ rows_all,
                                                      int max_tuples, double mu_start, double delta, int delta_absolute,
                                                      double division_factor, int decrease_every, int iterations,
                                                      double* __restrict__ T_out, int* __restrict__ info,
                                                      double* __restrict__ weights_out, double* __restrict__ norm_all)
{
    __shared__ double red[FGR_WAVES * FGR_NV];
    __shared__ double sh[24];                                    // c_src 0..2, c_tgt 3..5, D 6, go 7, T 8..19, failed 20
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* src_off = meta, *tgt_off = meta + (npairs + 1);
    const int ns = src_off[b + 1] - src_off[b], nt = tgt_off[b + 1] - tgt_off[b];
    const float* S = src + 3 * (size_t)src_off[b], *Tg = tgt + 3 * (size_t)tgt_off[b];
    const int* rows = rows_all + (size_t)b * 6 * max_tuples;
    const int m = 3 * info[4 * b + 1];                           // kept rows (k_fgr_tuples)
    double* W = weights_out ? weights_out + (size_t)b * 3 * max_tuples : nullptr;
    double* N = norm_all + (size_t)b * 18 * max_tuples;          // per row: normalised source point, normalised target point
    const double nan = __builtin_nan("");
    if (W)
        for (int i = tid; i < 3 * max_tuples; i += FGR_W) W[i] = nan;

    // normalisation
    double c[3], cnt;
    fgr_mean(S, ns, red, c, cnt);
    if (tid == 0) { sh[0] = c[0]; sh[1] = c[1]; sh[2] = c[2]; sh[7] = cnt > 0.0 ? 1.0 : 0.0; }
    fgr_mean(Tg, nt, red, c, cnt);
    if (tid == 0) { sh[3] = c[0]; sh[4] = c[1]; sh[5] = c[2]; if (!(cnt > 0.0)) sh[7] = 0.0; }
    __syncthreads();
    double D = 0.0;
    if (sh[7] != 0.0) {                                          // (block-uniform)
        double v[1] = { fmax(fgr_max_norm2(S, ns, sh), fgr_max_norm2(Tg, nt, sh + 3)) };
        for (int d = WAVE / 2; d > 0; d >>= 1) v[0] = fmax(v[0], __shfl_xor(v[0], d, WAVE));
        __syncthreads();
        if (tid % WAVE == 0) red[tid / WAVE] = v[0];
        __syncthreads();
        if (tid == 0) sh[6] = sqrt(fmax(fmax(red[0], red[1]), fmax(red[2], red[3])));
        __syncthreads();
        D = sh[6];
    }
    const bool go = sh[7] != 0.0 && D > 0.0 && m >= FGR_MIN_ROWS;
    if (tid == 0) {
        for (int k = 0; k < 12; k++) sh[8 + k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        sh[20] = 0.0;
    }
    __syncthreads();
    int status = BUF_FGR_NOTHING, updates = 0;
    if (go) {
        status = BUF_FGR_OK;
        for (int i = tid; i < m; i += FGR_W) {
            const int is = rows[2 * i], it = rows[2 * i + 1];
            for (int k = 0; k < 3; k++) {
                N[6 * (size_t)i + k] = ((double)S[3 * (size_t)is + k] - sh[k]) / D;
                N[6 * (size_t)i + 3 + k] = ((double)Tg[3 * (size_t)it + k] - sh[3 + k]) / D;
            }
        }
        double mu = mu_start;
        const double floor_mu = delta_absolute ? (delta / D) * (delta / D) : delta;
        for (int iter = 0; iter < iterations; iter++) {
            double T[12];
#pragma unroll
            for (int k = 0; k < 12; k++) T[k] = sh[8 + k];
            double v[FGR_NV];
#pragma unroll
            for (int k = 0; k < FGR_NV; k++) v[k] = 0.0;
            for (int i = tid; i < m; i += FGR_W) {               // each lane reads what it wrote itself: no fence needed
                const double* e = N + 6 * (size_t)i;
                const double sx = e[0], sy = e[1], sz = e[2];
                const double q[3] = { ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[9], ((T[3] * sx + T[4] * sy) + T[5] * sz) + T[10],
                                      ((T[6] * sx + T[7] * sy) + T[8] * sz) + T[11] };
                const double r[3] = { e[3] - q[0], e[4] - q[1], e[5] - q[2] };
                const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                double w = 0.0;
                if (isfinite(rr)) { const double f = mu / (rr + mu); w = f * f; }
                if (W) W[i] = w;
                if (w == 0.0) continue;
                // the three Jacobian rows
                const double J[3][6] = { { 0.0, -q[2], q[1], -1.0, 0.0, 0.0 }, { q[2], 0.0, -q[0], 0.0, -1.0, 0.0 },
                                         { -q[1], q[0], 0.0, 0.0, 0.0, -1.0 } };
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int bb = a; bb < 6; bb++) {
                        v[k] += w * ((J[0][a] * J[0][bb] + J[1][a] * J[1][bb]) + J[2][a] * J[2][bb]);
                        k++;
                    }
#pragma unroll
                for (int a = 0; a < 6; a++) v[21 + a] += w * ((J[0][a] * r[0] + J[1][a] * r[1]) + J[2][a] * r[2]);
            }
            tile_sum<FGR_NV, FGR_WAVES, false>(v, red);
            if (tid == 0) {
                double x[6];
                if (solve6(v, v + 21, x)) fgr_apply(x, sh + 8);
                else sh[20] = 1.0;
            }
            __syncthreads();
            if (sh[20] != 0.0) { status = BUF_FGR_FAILED; break; }      // (block-uniform)
            updates++;
            if (iter % decrease_every == 0 && mu > floor_mu) mu /= division_factor;
        }
    }
    if (tid != 0) return;
    double* To = T_out + 16 * (size_t)b;
    for (int k = 0; k < 16; k++) To[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (updates > 0) {                                           // T_out = [R | D t + c_tgt - R c_src]
        const double* T = sh + 8;
        for (int r = 0; r < 3; r++) {
            for (int cc = 0; cc < 3; cc++) To[4 * r + cc] = T[3 * r + cc];
            const double rc = (T[3 * r] * sh[0] + T[3 * r + 1] * sh[1]) + T[3 * r + 2] * sh[2];
            To[4 * r + 3] = (D * T[9 + r] + sh[3 + r]) - rc;
        }
    }
    info[4 * b] = status;
    info[4 * b + 3] = updates;
}

// ------------------------------------------------------------------------------------------
struct FgrWs { int* meta; int* rows; double* norm; };

static FgrWs carve_fgr(WsCarver& w, int npairs, int max_tuples)
{
    FgrWs e;
    e.meta = w.take<int>(5 * (size_t)npairs + 3);
    e.rows = w.take<int>((size_t)npairs * 6 * max_tuples);
    e.norm = w.take<double>((size_t)npairs * 18 * max_tuples);
    return e;
}

extern "C" size_t buf_fgr_ws_bytes(int n_corr_total, int npairs, int max_tuples)
{
    if (n_corr_total < 0 || npairs <= 0 || max_tuples < 1 || max_tuples > FGR_MAX_TUPLES) return 0;
    WsCarver w(nullptr, 0);
    carve_fgr(w, npairs, max_tuples);
    return w.used();
}

// The (src, tgt, corr) batch of buf_fgr_batched, buf_sc2_batched and buf_clique_batched (fn = the entry point's name), in the order
// all three test it: null host arrays (more_host: the entry point's further ones), null outputs, per pair a negative length and
// then the entry point's own limit (pair_limit(b) sets the error and returns its code), the int32 totals, null inputs.
// nct = correspondences of the batch, maxn = the most in one pair.
template <class PairLimit>
static int corr_batch_check(const char* fn, const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                            const int* corr, const int* corr_lengths_host, int npairs, bool more_host, const void* T_out,
                            const void* info_out, long long& nct, long long& maxn, PairLimit pair_limit)
{
    BUF_REQUIRE(src_lengths_host && tgt_lengths_host && corr_lengths_host && more_host, BUF_EINVAL, "%s: null host array", fn);
    BUF_REQUIRE(T_out && info_out, BUF_EINVAL, "%s: null output", fn);
    long long nst = 0, ntt = 0;
    nct = maxn = 0;
    for (int b = 0; b < npairs; b++) {
        BUF_REQUIRE(src_lengths_host[b] >= 0 && tgt_lengths_host[b] >= 0 && corr_lengths_host[b] >= 0, BUF_EINVAL,
                    "%s: negative length in pair %d", fn, b);
        if (const int rc = pair_limit(b)) return rc;
        nst += src_lengths_host[b]; ntt += tgt_lengths_host[b]; nct += corr_lengths_host[b];
        maxn = corr_lengths_host[b] > maxn ? corr_lengths_host[b] : maxn;
    }
    BUF_REQUIRE(nst < 0x7fffffffLL && ntt < 0x7fffffffLL && nct < 0x7fffffffLL, BUF_EINVAL,
                "%s: %lld / %lld points, %lld correspondences (int32 indices)", fn, nst, ntt, nct);
    BUF_REQUIRE((nst == 0 || src) && (ntt == 0 || tgt) && (nct == 0 || corr), BUF_EINVAL, "%s: null input", fn);
    return BUF_OK;
}

extern "C" int buf_fgr_batched(const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                               const int* corr, const int* corr_lengths_host, int npairs, const unsigned long long* seeds_host,
                               double tuple_scale, int max_tuples, int trial_factor, double mu_start, double delta, int delta_absolute,
                               double division_factor, int decrease_every, int iterations, double* T_out, int* info_out, int* rows_out,
                               double* weights_out, void* ws, size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(npairs >= 0, BUF_EINVAL, "buf_fgr_batched: npairs=%d", npairs);
    BUF_REQUIRE(tuple_scale > 0.0 && tuple_scale <= 1.0, BUF_EINVAL, "buf_fgr_batched: tuple_scale=%g (must be in (0, 1])", tuple_scale);
    BUF_REQUIRE(max_tuples >= 1 && max_tuples <= FGR_MAX_TUPLES, BUF_EINVAL, "buf_fgr_batched: max_tuples=%d (1..%d)", max_tuples,
                FGR_MAX_TUPLES);
    BUF_REQUIRE(trial_factor >= 1, BUF_EINVAL, "buf_fgr_batched: trial_factor=%d", trial_factor);
    BUF_REQUIRE(mu_start > 0.0 && mu_start <= 1.7976931348623157e308, BUF_EINVAL, "buf_fgr_batched: mu_start=%g (must be finite and > 0)",
                mu_start);
    BUF_REQUIRE(delta > 0.0 && delta <= 1.7976931348623157e308, BUF_EINVAL, "buf_fgr_batched: delta=%g (must be finite and > 0)", delta);
    BUF_REQUIRE(division_factor > 1.0 && division_factor <= 1.7976931348623157e308, BUF_EINVAL,
                "buf_fgr_batched: division_factor=%g (must be finite and > 1)", division_factor);
    BUF_REQUIRE(decrease_every >= 1 && iterations >= 0, BUF_EINVAL, "buf_fgr_batched: decrease_every=%d iterations=%d", decrease_every,
                iterations);
    if (npairs == 0) return BUF_OK;
    long long nct, maxn;
    const int brc = corr_batch_check("buf_fgr_batched", src, src_lengths_host, tgt, tgt_lengths_host, corr, corr_lengths_host, npairs,
                                     seeds_host != nullptr, T_out, info_out, nct, maxn, [&](int b) {
        BUF_REQUIRE((long long)trial_factor * corr_lengths_host[b] <= 0x7fffffffLL, BUF_EINVAL,
                    "buf_fgr_batched: trial_factor * %d correspondences of pair %d overflows int", corr_lengths_host[b], b);
        return (int)BUF_OK;
    });
    if (brc) return brc;
    const size_t need = buf_fgr_ws_bytes((int)nct, npairs, max_tuples);
    BUF_REQUIRE(ws && ws_bytes >= need, BUF_EINVAL, "buf_fgr_batched: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);

    WsCarver w(ws, ws_bytes);
    const FgrWs e = carve_fgr(w, npairs, max_tuples);
    const size_t B = (size_t)npairs;
    int* meta = (int*)malloc(sizeof(int) * (5 * B + 3));
    BUF_REQUIRE(meta, BUF_EINVAL, "buf_fgr_batched: out of host memory");
    int* so = meta, *to = meta + (B + 1), *co = meta + 2 * (B + 1), *sd = meta + 3 * (B + 1);
    so[0] = to[0] = co[0] = 0;
    for (size_t b = 0; b < B; b++) {
        so[b + 1] = so[b] + src_lengths_host[b];
        to[b + 1] = to[b] + tgt_lengths_host[b];
        co[b + 1] = co[b] + corr_lengths_host[b];
        sd[2 * b] = (int)(unsigned int)(seeds_host[b] & 0xffffffffull);
        sd[2 * b + 1] = (int)(unsigned int)(seeds_host[b] >> 32);
    }
    const int rc = upload_ints(e.meta, meta, (long long)(5 * B + 3), "buf_fgr_batched", s);
    free(meta);
    if (rc) return rc;
    int* rows = rows_out ? rows_out : e.rows;
    k_fgr_tuples<<<npairs, FGR_W, 0, s>>>(src, tgt, corr, e.meta, npairs, tuple_scale * tuple_scale, max_tuples, trial_factor, rows,
                                          info_out);
    k_fgr_optimize<<<npairs, FGR_W, 0, s>>>(src, tgt, e.meta, npairs, rows, max_tuples, mu_start, delta, delta_absolute, division_factor,
                                            decrease_every, iterations, T_out, info_out, weights_out, e.norm);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
