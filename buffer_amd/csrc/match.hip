// N12  Batched descriptor matching: the exact nearest and second-nearest row of the other side for every row of both sides of every
// pair, then the mutual and ratio filters and an ordered compaction (the contract is in include/buffer_hip.h).
//
//   k_match_scan<W>  ONE launch for both directions of all pairs.  The host lays the workgroups out as segments (pair p, direction 0:
//                    rows of A query B; direction 1: rows of B query A), ceil(rows / 64) workgroups each; a workgroup finds its segment
//                    in the prefix table by bisection.  Four wavefronts own 64 query rows: lane = query, its vector in W registers
//                    (W = d padded to a multiple of 4 with zeros: a zero dimension adds +0 to a sum).  The other side's rows pass through
//                    an LDS tile (256 rows at W <= 36: 32 / 36 KB, 128 rows at W = 64: 32 KB; with the 4 KB merge buffer four
//                    workgroups fit the 160 KB of a CU), read as float4 broadcasts; wavefront w takes the rows w, w + 4, ...; every
//                    lane keeps its smallest and second smallest key; the four are merged through LDS by wavefront 0.  A non-finite
//                    component becomes NaN on its way into the tile, so a row with one has a NaN sum against every finite query and
//                    is left out (finite rows give sums in [0, +inf], never NaN); a non-finite query writes two empty keys.
//   k_match_select   one workgroup per pair: the keep flag of every row of A (has a neighbour, mutual, ratio), nn_out / ssd_out, the
//                    pair's count.
//   k_match_scatter  one workgroup per pair: its first output row = the sum of the counts of the pairs before it, then its kept rows
//                    in ascending i (ballot prefixes, 256 rows a trip).
// No atomics anywhere and every minimum is over distinct keys: a pair's rows are the same bits alone, in any batch, at every launch.
#include "common.h"

#define MATCH_Q 64
#define MATCH_WAVES 4
#define MATCH_T (MATCH_WAVES * WAVE)
#define MATCH_NONE (~0ull)

// (k1, k2) = the two smallest of {k1, k2, key}, k1 <= k2 kept
__device__ __forceinline__ void match_take(unsigned long long key, unsigned long long& k1, unsigned long long& k2)
{
    const bool lt = key < k1;
    const unsigned long long hi = lt ? k1 : key;
    k1 = lt ? key : k1;
    k2 = hi < k2 ? hi : k2;
}

__device__ __forceinline__ bool match_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

template <int W>
__global__ void __launch_bounds__(MATCH_T) k_match_scan(const float* __restrict__ fa, const float* __restrict__ fb,
                                                        const int* __restrict__ meta, int pairs, int d,
                                                        unsigned long long* __restrict__ best_a, unsigned long long* __restrict__ best_b)
{
    constexpr int ROWS = W <= 36 ? 256 : 128, W4 = W / 4;
    __shared__ float4 tile[ROWS * W4];
    __shared__ unsigned long long red[MATCH_WAVES][2][WAVE];
    const int* aoff = meta;
    const int* boff = meta + (pairs + 1);
    const int* seg_off = meta + 2 * (pairs + 1);                  // [2 pairs + 1]: first workgroup of segment 2 p + direction
    // XCD-contiguous block order: the workgroups of one pair stream the same rows and meet in one L2
    const int lb = xcd_contiguous_block((int)blockIdx.x, (int)gridDim.x);
    const int seg = find_elem(seg_off, 2 * pairs, lb);            // (empty segments own no workgroup: the last of equal offsets wins)
    const int p = seg >> 1, dir = seg & 1;
    const int a0 = aoff[p], na = aoff[p + 1] - a0, b0 = boff[p], nb = boff[p + 1] - b0;
    const int nq = dir ? nb : na, nr = dir ? na : nb;
    const float* Q = dir ? fb + (size_t)b0 * d : fa + (size_t)a0 * d;
    const float* R = dir ? fa + (size_t)a0 * d : fb + (size_t)b0 * d;
    unsigned long long* out = dir ? best_b + 2 * (size_t)b0 : best_a + 2 * (size_t)a0;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int q0 = (lb - seg_off[seg]) * MATCH_Q;                 // < nq: the segment has ceil(nq / 64) workgroups
    const int q = q0 + lane;
    const bool active = q < nq;

    float qv[W];
    const float* qp = Q + (size_t)(active ? q : q0) * d;
    bool qfin = true;
#pragma unroll
    for (int c = 0; c < W; c++) {
        qv[c] = c < d ? qp[c] : 0.f;
        qfin = qfin && match_finite(qv[c]);
    }

    unsigned long long k1 = MATCH_NONE, k2 = MATCH_NONE;
    float* tf = reinterpret_cast<float*>(tile);
    for (int base = 0; base < nr; base += ROWS) {
        const int cnt = min(ROWS, nr - base);
        __syncthreads();                                          // the tile before this one is read out
        for (int t = threadIdx.x; t < cnt * W; t += MATCH_T) {
            const int r = t / W, c = t - r * W;
            float v = 0.f;
            if (c < d) {
                v = R[(size_t)(base + r) * d + c];
                if (!match_finite(v)) v = __uint_as_float(0x7fc00000u);
            }
            tf[t] = v;
        }
        __syncthreads();
        for (int i = w; i < cnt; i += MATCH_WAVES) {
            float ssd = 0.f;
#pragma unroll
            for (int c4 = 0; c4 < W4; c4++) {
                const float4 r = tile[i * W4 + c4];
                const float t0 = __fsub_rn(qv[4 * c4], r.x);     ssd = __fadd_rn(ssd, __fmul_rn(t0, t0));
                const float t1 = __fsub_rn(qv[4 * c4 + 1], r.y); ssd = __fadd_rn(ssd, __fmul_rn(t1, t1));
                const float t2 = __fsub_rn(qv[4 * c4 + 2], r.z); ssd = __fadd_rn(ssd, __fmul_rn(t2, t2));
                const float t3 = __fsub_rn(qv[4 * c4 + 3], r.w); ssd = __fadd_rn(ssd, __fmul_rn(t3, t3));
            }
            const unsigned long long key =
                ssd == ssd ? (((unsigned long long)__float_as_uint(ssd) << 32) | (unsigned int)(base + i)) : MATCH_NONE;
            match_take(key, k1, k2);
        }
    }
    red[w][0][lane] = k1;
    red[w][1][lane] = k2;
    __syncthreads();
    if (w == 0 && active) {
        for (int i = 1; i < MATCH_WAVES; i++) {                   // a fixed order (and the two smallest of distinct keys have none)
            match_take(red[i][0][lane], k1, k2);
            match_take(red[i][1][lane], k1, k2);
        }
        if (!qfin) k1 = k2 = MATCH_NONE;
        out[2 * (size_t)q] = k1;
        out[2 * (size_t)q + 1] = k2;
    }
}

// sum of v over the workgroup's 256 threads, the same value in every thread; red holds MATCH_WAVES ints
__device__ __forceinline__ int match_block_sum(int v, int* red)
{
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    __syncthreads();                                              // red may still be read from the call before
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    int s = 0;
    for (int i = 0; i < MATCH_WAVES; i++) s += red[i];
    return s;
}

__global__ void __launch_bounds__(MATCH_T) k_match_select(const int* __restrict__ meta, int pairs,
                                                          const unsigned long long* __restrict__ best_a,
                                                          const unsigned long long* __restrict__ best_b, int mutual, int use_ratio,
                                                          float r2, unsigned char* __restrict__ keep, int* __restrict__ counts,
                                                          int* __restrict__ nn_out, float* __restrict__ ssd_out)
{
    __shared__ int red[MATCH_WAVES];
    const int p = blockIdx.x;
    const int a0 = meta[p], na = meta[p + 1] - a0, b0 = meta[pairs + 1 + p];
    int cnt = 0;
    for (int i = threadIdx.x; i < na; i += MATCH_T) {
        const size_t row = (size_t)a0 + i;
        const unsigned long long k1 = best_a[2 * row], k2 = best_a[2 * row + 1];
        const float s1 = __uint_as_float((unsigned int)(k1 >> 32)), s2 = __uint_as_float((unsigned int)(k2 >> 32));
        bool ok = k1 != MATCH_NONE;
        if (ok && mutual) {
            const unsigned long long kb = best_b[2 * ((size_t)b0 + (unsigned int)k1)];
            ok = kb != MATCH_NONE && (unsigned int)kb == (unsigned int)i;
        }
        if (ok && use_ratio && k2 != MATCH_NONE) ok = s1 <= __fmul_rn(r2, s2);
        keep[row] = ok ? 1 : 0;
        cnt += ok ? 1 : 0;
        if (nn_out) {
            nn_out[2 * row] = k1 != MATCH_NONE ? (int)(unsigned int)k1 : -1;
            nn_out[2 * row + 1] = k2 != MATCH_NONE ? (int)(unsigned int)k2 : -1;
        }
        if (ssd_out) {
            ssd_out[2 * row] = k1 != MATCH_NONE ? s1 : __uint_as_float(0x7f800000u);
            ssd_out[2 * row + 1] = k2 != MATCH_NONE ? s2 : __uint_as_float(0x7f800000u);
        }
    }
    cnt = match_block_sum(cnt, red);
    if (threadIdx.x == 0) counts[p] = cnt;
}

__global__ void __launch_bounds__(MATCH_T) k_match_scatter(const int* __restrict__ meta, int pairs,
                                                           const unsigned long long* __restrict__ best_a,
                                                           const unsigned char* __restrict__ keep, const int* __restrict__ counts,
                                                           int* __restrict__ corr_out)
{
    __shared__ int red[MATCH_WAVES];
    const int p = blockIdx.x;
    const int a0 = meta[p], na = meta[p + 1] - a0;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    int before = 0;
    for (int t = threadIdx.x; t < p; t += MATCH_T) before += counts[t];
    long long o = match_block_sum(before, red);                    // (the total is at most the rows of A: an int)
    for (int i0 = 0; i0 < na; i0 += MATCH_T) {
        const int i = i0 + threadIdx.x;
        const bool hit = i < na && keep[(size_t)a0 + i] != 0;
        const unsigned long long has = __ballot(hit);
        __syncthreads();                                          // red is read out
        if (lane == 0) red[w] = __popcll(has);
        __syncthreads();
        int lower = 0, all = 0;
        for (int j = 0; j < MATCH_WAVES; j++) {
            lower += j < w ? red[j] : 0;
            all += red[j];
        }
        if (hit) {
            const size_t dst = (size_t)(o + lower + __popcll(has & ((1ull << lane) - 1ull)));
            corr_out[2 * dst] = i;
            corr_out[2 * dst + 1] = (int)(unsigned int)best_a[2 * ((size_t)a0 + i)];
        }
        o += all;
    }
}

struct MatchWs { int* meta; unsigned long long* best_a; unsigned long long* best_b; unsigned char* keep; };

static MatchWs carve_match(WsCarver& w, long long na_total, long long nb_total, int pairs)
{
    MatchWs e;
    e.meta = w.take<int>(4 * (size_t)pairs + 3);                  // aoff[P + 1] | boff[P + 1] | seg_off[2 P + 1]
    e.best_a = w.take<unsigned long long>(2 * (size_t)na_total);
    e.best_b = w.take<unsigned long long>(2 * (size_t)nb_total);
    e.keep = w.take<unsigned char>((size_t)na_total);
    return e;
}

extern "C" size_t buf_feature_match_ws_bytes(long long na_total, long long nb_total, int pairs)
{
    if (na_total < 0 || nb_total < 0 || pairs < 0) return 256;
    WsCarver w(nullptr, 0);
    carve_match(w, na_total, nb_total, pairs);
    return w.used() + 256;
}

extern "C" int buf_feature_match(const float* fa, const int* a_lengths_host, const float* fb, const int* b_lengths_host, int pairs, int d,
                                 int mutual, float ratio, int* corr_out, int* counts_out, int* nn_out, float* ssd_out, void* ws,
                                 size_t ws_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(pairs >= 0, BUF_EINVAL, "buf_feature_match: pairs=%d", pairs);
    BUF_REQUIRE(d >= 1 && d <= 64, BUF_EINVAL, "buf_feature_match: d=%d (1..64)", d);
    BUF_REQUIRE(ratio < 1.f, BUF_EINVAL, "buf_feature_match: ratio=%g (must be below 1; <= 0 switches the test off)", (double)ratio);
    if (pairs == 0) return BUF_OK;
    BUF_REQUIRE(a_lengths_host && b_lengths_host, BUF_EINVAL, "buf_feature_match: null host array");
    BUF_REQUIRE(counts_out, BUF_EINVAL, "buf_feature_match: null output counts_out");
    long long nat = 0, nbt = 0, blocks = 0;
    for (int p = 0; p < pairs; p++) {
        BUF_REQUIRE(a_lengths_host[p] >= 0 && b_lengths_host[p] >= 0, BUF_EINVAL, "buf_feature_match: negative length in pair %d", p);
        nat += a_lengths_host[p];
        nbt += b_lengths_host[p];
        blocks += cdiv(a_lengths_host[p], MATCH_Q) + cdiv(b_lengths_host[p], MATCH_Q);
    }
    BUF_REQUIRE(nat < 0x7fffffffLL && nbt < 0x7fffffffLL, BUF_EINVAL, "buf_feature_match: %lld / %lld rows (int32 indices)", nat, nbt);
    BUF_REQUIRE((nat == 0 || fa) && (nbt == 0 || fb), BUF_EINVAL, "buf_feature_match: null input");
    BUF_REQUIRE(nat == 0 || corr_out, BUF_EINVAL, "buf_feature_match: null output corr_out");
    if (nat == 0) {                                               // no row of A: no correspondence, nothing to scan for
        BUF_CHECK_HIP(hipMemsetAsync(counts_out, 0, sizeof(int) * (size_t)pairs, s));
        return BUF_OK;
    }
    const size_t need = buf_feature_match_ws_bytes(nat, nbt, pairs);
    BUF_REQUIRE(ws && ws_bytes >= need, BUF_EINVAL, "buf_feature_match: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);

    WsCarver wc(ws, ws_bytes);
    const MatchWs e = carve_match(wc, nat, nbt, pairs);
    const size_t P = (size_t)pairs;
    int* meta = (int*)malloc(sizeof(int) * (4 * P + 3));
    BUF_REQUIRE(meta, BUF_EINVAL, "buf_feature_match: out of host memory");
    int* ao = meta, *bo = meta + (P + 1), *so = meta + 2 * (P + 1);
    ao[0] = bo[0] = so[0] = 0;
    for (size_t p = 0; p < P; p++) {
        ao[p + 1] = ao[p] + a_lengths_host[p];
        bo[p + 1] = bo[p] + b_lengths_host[p];
        so[2 * p + 1] = so[2 * p] + cdiv(a_lengths_host[p], MATCH_Q);
        so[2 * p + 2] = so[2 * p + 1] + cdiv(b_lengths_host[p], MATCH_Q);
    }
    const int rc = upload_ints(e.meta, meta, (long long)(4 * P + 3), "buf_feature_match", s);
    free(meta);
    if (rc) return rc;
    const unsigned int grid = (unsigned int)blocks;               // >= 1: A has a row
    if (d <= 32) k_match_scan<32><<<grid, MATCH_T, 0, s>>>(fa, fb, e.meta, pairs, d, e.best_a, e.best_b);
    else if (d <= 36) k_match_scan<36><<<grid, MATCH_T, 0, s>>>(fa, fb, e.meta, pairs, d, e.best_a, e.best_b);
    else k_match_scan<64><<<grid, MATCH_T, 0, s>>>(fa, fb, e.meta, pairs, d, e.best_a, e.best_b);
    const bool use_ratio = ratio > 0.f;
    const float r2 = use_ratio ? (float)((double)ratio * (double)ratio) : 0.f;
    k_match_select<<<pairs, MATCH_T, 0, s>>>(e.meta, pairs, e.best_a, e.best_b, mutual != 0, use_ratio, r2, e.keep, counts_out, nn_out,
                                             ssd_out);
    k_match_scatter<<<pairs, MATCH_T, 0, s>>>(e.meta, pairs, e.best_a, e.keep, counts_out, corr_out);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
