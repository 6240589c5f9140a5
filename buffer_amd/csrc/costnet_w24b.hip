// A13 -- the second forms of layers 1 and 3 of the fused fp32 cost net (cw24b_layer1, cw24b_layer3), which cost_net_body
// (csrc/costnet_body.hip) runs where CostNetParams::f24[3] / f24[4] hold the layer's F(2x4) set:
//
//   layer 1 (96 -> 64, 18 x 18 -> 16 x 16)    F(2x4, 3x3) tiles: 8 x 4 = 32 tiles in exactly two M-tiles, 2 x 24 = 48 matrix instructions per
//                                             (k-step, N-tile) instead of the 64 of F(2x2): 6 144 -> 4 608 per match, no padded lane
//   layer 3 (64 -> 128, 14 x 14 -> 12 x 12)   a hybrid: 5 x 3 = 15 F(2x4) tiles in ONE M-tile (output rows 0..9, 24 per unit) and the last
//                                             tile row (output rows 10, 11) in F(2x2) (16 per unit): 40 instead of 48, 6 144 -> 5 120
// 26 608 (the forms of csrc/costnet_w24.hip in layers 2, 4 and 6) -> 24 048 matrix instructions per match.
//
// Layer 1 keeps ONE k' plane of the layer-0 activation resident at a time: 32 channels x 18 rows, channel-major [32][CWB_CS1] with rows of
// CWB_RS1 words, formed once per plane (18 rows per plane; the chunked F(2x2) form makes 24 row formations over its four overlapping
// chunks).  Wavefront (p, j) owns the N-tile pair p over M-tile j = tile rows 4j..4j+3 = output rows 8j..8j+7.  A plane is 8 k-steps = one
// round of two iterations per row component; the folded outputs of the three planes add up in the wavefront's 64 held registers (the bias
// rides in plane 0), so no partial sum passes between wavefronts, and they are stored behind the barrier that ends the last plane's reads:
// the output map [64][CW_CS1] covers the layer-0 maps SM / TB.
//
// Banks of layer 1's window reads (ds_read_b64: a half-wave = 16 tiles x 2 channels per pass over the 64 banks).  With rows of 18 words the
// tile rows 0 and 2 of an M-tile lie 72 = 8 mod 64 words apart and collide two-way with the tile columns 2, 3.  Rows of 24 words put the
// four tile rows at 0, 48, 96 = 32, 144 = 16 mod 64, the four tile columns at +0, 4, 8, 12: the 16 windows of a read take the bank pairs
// {4i, 4i + 1}, i = 0..15, and the channel stride 450 = 2 mod 64 puts the half-wave's second channel on {4i + 2, 4i + 3}: conflict-free.
// 32 x 450 = 14 400 floats end in front of SM (16 376).  The last window is columns 12..17 of an 18-column row: no overread, no clear.
//
// Layer 3: one w24_round over the whole K = 64 with cw24_layer's addressing at HIN = 14, NTX = 3, TYPM = 5 (the last window ends at column
// 13 of a 14-word row: no overread), then the round of cw_layer's M-tile 2 (tile rows 4, 5) on the existing F(2x2) set, of which only
// tile row 5 is stored.  All outputs wait for the barrier that ends the reads.
//
// Every layer is switched by its filter set: a null set runs the layer's F(2x2) form of csrc/costnet.hip (layer 1: in four chunks).
#include "common.h"

#ifndef CWB_RS1           // (a development build may pass another pair, e.g. the compact -DCWB_RS1=18 -DCWB_CS1=326: profiles/cost_f24b_ab.md)
#define CWB_RS1 24        // row and channel stride of layer 1's resident k' plane (see the bank plan above)
#define CWB_CS1 450
#endif
static_assert(32 * CWB_CS1 <= CVA_SM, "the plane ends in front of the layer-0 maps");
static_assert(17 * CWB_RS1 + 4 * 3 + 6 <= CWB_CS1 && CWB_RS1 % 2 == 0 && CWB_CS1 % 2 == 0, "the last window stays inside the channel; ds_read_b64");
static_assert(64 * CW_CS1 <= CV_BUF, "layer 1's output map");

// all 18 rows n' of plane kq: X[c][n' * CWB_RS1 + l'] = relu(Smap[kq][(l' - n') mod 20][c] + Tb[kq][l'][c])
__device__ __forceinline__ void cw24b_form_plane(float* __restrict__ X, const float* __restrict__ SM, const float* __restrict__ TB, int kq)
{
    for (int i = threadIdx.x; i < 324 * 8; i += CV_THREADS) {
        const int c4 = i & 7, pos = i >> 3, n = pos / 18, lq = pos - n * 18;
        int j = lq - n;
        j = j < 0 ? j + 20 : j;
        const cvx4 sv = *reinterpret_cast<const cvx4*>(SM + (kq * 20 + j) * CV_C32 + c4 * 4);
        const cvx4 tv = *reinterpret_cast<const cvx4*>(TB + (kq * 18 + lq) * CV_C32 + c4 * 4);
        float* d = X + c4 * 4 * CWB_CS1 + n * CWB_RS1 + lq;
#pragma unroll
        for (int q = 0; q < 4; q++) d[q * CWB_CS1] = fmaxf(sv[q] + tv[q], 0.f);
    }
}

// w24_round (csrc/convnet_w24.hip) whose folded outputs ADD to Y, with the accumulators cleared before every pass: s_I = the column
// transform of row component I alone,
//     pass 0: row 0 += s_0     pass 1: row 0 += s_1, row 1 += s_1     pass 2: row 0 += s_2, row 1 -= s_2     pass 3: row 1 -= s_3
// (w24_round lets the accumulators run on through the passes and takes row 1 = -F_0 + 2 F_1 - F_3 from the running sums F_I.  Summed
// plane by plane that order leaves three times the folds of sums that cancel: restated in float32 it came to 5.6e-5 on the golden
// matches, this order to 1.3e-5 -- tools/cost_f24b_restate.py.)  The bias rides in column component 1 of pass 1, which both rows take
// once.  bias_lane may be null (the planes behind the first).
template <unsigned KSTEP>
__device__ __forceinline__ void cw24b_round_add(unsigned (&RA)[4], __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned wp_after, unsigned lofs4, unsigned lofs2,
                                                int niter, unsigned pstride, const float* __restrict__ bias_lane, wgf4 (&W4)[2][2], wgf2 (&W2)[2][2],
                                                wgf4 (&Y)[2][2][4])
{
    using std::integral_constant;
    wgf2 D[2][6];
    wgf4 bv[2];
#pragma unroll
    for (int n = 0; n < 2; n++) bv[n] = bias_lane ? *reinterpret_cast<const wgf4*>(bias_lane + n * 16) : (wgf4){ 0.f, 0.f, 0.f, 0.f };
    wgf4 acc[2][6];
    float zero = 0.f;
    asm volatile("" : "+v"(zero));                   // (an opaque zero: see wg_round)
    auto run = [&](auto ic) __attribute__((always_inline)) {
        constexpr int I = decltype(ic)::value;
        constexpr int INEXT = I == 3 ? 0 : I + 1;
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int j = 0; j < 6; j++) acc[n][j] = (I == 1 && j == 1) ? bv[n] : (wgf4){ zero, zero, zero, zero };
        constexpr int ICHAIN = (INEXT != 0 && wg_chains(I)) ? INEXT : -1;
        w24_pass<I, wg_chains(I - 1), ICHAIN, KSTEP>(RA, rs, wp + I * pstride, INEXT == 0 ? wp_after : wp + (I + 1) * pstride, lofs4, lofs2, niter, W4, W2, acc, D);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 2; n++) {
            wgf4 f[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {            // A4^T as in w24_round
                const float p = acc[n][1][r] + acc[n][2][r], q = acc[n][1][r] - acc[n][2][r];
                const float t = acc[n][3][r] + acc[n][4][r], d = acc[n][3][r] - acc[n][4][r];
                f[0][r] = acc[n][0][r] + p + t;
                f[1][r] = __builtin_fmaf(2.f, d, q);
                f[2][r] = __builtin_fmaf(4.f, t, p);
                f[3][r] = __builtin_fmaf(8.f, d, q) + acc[n][5][r];
            }
#pragma unroll
            for (int v = 0; v < 4; v++) {
                if constexpr (I <= 2) Y[n][0][v] += f[v];
                if constexpr (I == 1) Y[n][1][v] += f[v];
                if constexpr (I >= 2) Y[n][1][v] -= f[v];
                if constexpr (I <= 2) asm volatile("" : "+v"(Y[n][0][v]));      // pinned here, as in w24_round
                if constexpr (I >= 1) asm volatile("" : "+v"(Y[n][1][v]));
            }
        }
    };
    run(integral_constant<int, 0>{});
    run(integral_constant<int, 1>{});
    run(integral_constant<int, 2>{});
    run(integral_constant<int, 3>{});
}

// Phase A.2 on F(2x4) tiles: from the layer-0 maps SM / TB to the layer-1 map [64][CW_CS1] at the buffer's start, barriers included.
__device__ __forceinline__ void cw24b_layer1(float* __restrict__ lds, const float* __restrict__ wt, const float* __restrict__ bias, int w)
{
    float* X = lds + CVA_XC;
    const float* SM = lds + CVA_SM;
    const float* TB = lds + CVA_TB;
    constexpr unsigned KSTEP = 16u * CWB_CS1;
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int pair = w & 1, t = w >> 1;
    unsigned RA[4];
    {
        const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)X;
        const int li = lane & 15, ty = 4 * t + (li >> 2), tx = li & 3;
#pragma unroll
        for (int a = 0; a < 4; a++) RA[a] = base + 4u * (unsigned)(lk * CWB_CS1 + (2 * ty + a) * CWB_RS1 + 4 * tx);
    }
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned pstride = 24u * W24_WSTRIDE;                            // [pair][i][k-step 0..23][...]: plane k' is the k-steps 8 k' .. 8 k' + 7
    const unsigned wp0 = (unsigned)pair * 4 * pstride;
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    const float* bv = bias + (2 * pair) * 16 + lk * 4;
    wgf4 W4[2][2];
    wgf2 W2[2][2];
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            W4[n][k] = wg_ldw(rs, wp0 + k * W24_WSTRIDE + n * 256, lofs4);
            W2[n][k] = w24_ldw2(rs, wp0 + k * W24_WSTRIDE + 512 + n * 128, lofs2);
        }
    wgf4 Y[2][2][4];
    {
        float zero = 0.f;
        asm volatile("" : "+v"(zero));
#pragma unroll
        for (int q = 0; q < 16; q++) Y[q >> 3][(q >> 2) & 1][q & 3] = (wgf4){ zero, zero, zero, zero };
    }
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        cw24b_form_plane(X, SM, TB, k);
        __syncthreads();
        const unsigned wp = wp0 + 8u * k * W24_WSTRIDE;
        cw24b_round_add<KSTEP>(RA, rs, wp, k < 2 ? wp + 8u * W24_WSTRIDE : wp0, lofs4, lofs2, 2, pstride, k == 0 ? bv : nullptr, W4, W2, Y);
        __syncthreads();                     // the plane may be overwritten; behind the last one the output map may cover SM / TB
    }
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));         // the store offsets are formed here, not kept from the layer's start
    const int li = lane_s & 15, ty = 4 * t + (li >> 2), tx = li & 3;
#pragma unroll
    for (int n = 0; n < 2; n++) {
        float* p = lds + ((2 * pair + n) * 16 + (lane_s >> 4) * 4) * CW_CS1 + 2 * ty * 16 + 4 * tx;
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                *reinterpret_cast<wgf4*>(p + r * CW_CS1 + u * 16) = (wgf4){ fmaxf(Y[n][u][0][r], 0.f), fmaxf(Y[n][u][1][r], 0.f), fmaxf(Y[n][u][2][r], 0.f), fmaxf(Y[n][u][3][r], 0.f) };
    }
    __syncthreads();
}

// Layer 3 over the map [64][CW_CS2] (14 x 14, rows of 14), rewritten in place as [128][CW_CS3] with rows of 12: wavefront w owns the N-tile
// pair w.  wt24: the layer's F(2x4) set, wt22: its F(2x2) set (group 2) as cw_layer reads it.
__device__ __forceinline__ void cw24b_layer3(float* __restrict__ map, const float* __restrict__ wt24, const float* __restrict__ wt22,
                                             const float* __restrict__ bias, int w)
{
    constexpr int HIN = 14, RS = 14, CS = CW_CS2, NTX = 3, TYPM = 5, CIN = 64, RSO = 12, CSO = CW_CS3, k4 = CIN / 4;
    static_assert((2 * (TYPM - 1) + 3) * RS + 4 * (NTX - 1) + 6 <= HIN * RS && RS % 2 == 0 && CS % 2 == 0, "the last F(2x4) window ends inside its row");
    constexpr unsigned KSTEP = 16u * CS;
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)map;
    unsigned RA[4];
    {
        const int li = lane & 15, q = li / NTX;
        int ty = q, tx = li - q * NTX;
        if (q >= TYPM) { ty = 0; tx = 0; }                                  // the idle lane recomputes tile (0, 0), never stored
#pragma unroll
        for (int a = 0; a < 4; a++) RA[a] = base + 4u * (unsigned)(lk * CS + (2 * ty + a) * RS + 4 * tx);
    }
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    const float* bv = bias + (2 * w) * 16 + lk * 4;
    wgf4 Y[2][2][4];
    {
        const __amdgpu_buffer_rsrc_t rs = wg_weights(wt24);
        const unsigned pstride = (unsigned)(k4 * W24_WSTRIDE);
        const unsigned wp = (unsigned)w * 4 * pstride;                     // [pair][i][k-step][...]
        wgf4 W4[2][2];
        wgf2 W2[2][2];
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                W4[n][k] = wg_ldw(rs, wp + k * W24_WSTRIDE + n * 256, lofs4);
                W2[n][k] = w24_ldw2(rs, wp + k * W24_WSTRIDE + 512 + n * 128, lofs2);
            }
        w24_round<false, KSTEP>(RA, rs, wp, wp, lofs4, lofs2, k4 >> 2, pstride, bv, W4, W2, Y);
    }
    // the F(2x2) tail: M-tile 2 of cw_layer<14, .., TYPM = 2>, tile rows 4 and 5 of six tiles each (lanes 12..15 recompute tile (0, 0))
    wgf4 Y2[2][3][2][2];
    {
        unsigned RB[3][4];
        const int li = lane & 15, q = li / 6;
        int ty = 4 + q, tx = li - q * 6;
        if (q >= 2) { ty = 0; tx = 0; }
#pragma unroll
        for (int a = 0; a < 4; a++) RB[0][a] = RB[1][a] = RB[2][a] = base + 4u * (unsigned)(lk * CS + (2 * ty + a) * RS + 2 * tx);
        const __amdgpu_buffer_rsrc_t rs = wg_weights(wt22);
        const unsigned wp = (unsigned)w * (CIN * 2 * 256);                 // [N-group][i 0..3][k-step][n2][lane][j]
        wgf4 W[2][2];
        wg_first_weights<2, 0, 2>(rs, wp, lofs4, 512, W);
        wg_round<2, 0, 1, KSTEP, true>(RB, rs, wp, wp, lofs4, k4 >> 2, 512, (unsigned)(k4 * 512), bv, W, Y2);
    }
    __syncthreads();                         // every wavefront has finished reading the map
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));         // the store offsets are formed here, not kept from the layer's start
    const int li = lane_s & 15;
    {
        const int q = li / NTX, tx = li - q * NTX;
        if (q < TYPM) {
#pragma unroll
            for (int n = 0; n < 2; n++) {
                float* p = map + ((2 * w + n) * 16 + (lane_s >> 4) * 4) * CSO + 2 * q * RSO + 4 * tx;
#pragma unroll
                for (int u = 0; u < 2; u++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        *reinterpret_cast<wgf4*>(p + r * CSO + u * RSO) = (wgf4){ fmaxf(Y[n][u][0][r], 0.f), fmaxf(Y[n][u][1][r], 0.f), fmaxf(Y[n][u][2][r], 0.f), fmaxf(Y[n][u][3][r], 0.f) };
            }
        }
    }
    if (li >= 6 && li < 12) {                // tile row 5 = output rows 10, 11
#pragma unroll
        for (int n = 0; n < 2; n++) {
            float* p = map + ((2 * w + n) * 16 + (lane_s >> 4) * 4) * CSO + 10 * RSO + 2 * (li - 6);
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    *reinterpret_cast<wgf2*>(p + r * CSO + u * RSO) = (wgf2){ fmaxf(Y2[n][0][u][0][r], 0.f), fmaxf(Y2[n][0][u][1][r], 0.f) };
        }
    }
}
