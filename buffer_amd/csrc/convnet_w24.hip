// A11 dense part -- w24_layer_pair, a layer form of the fused kernel (cyl_net_w25t_body, csrc/convnet_w25t.hip, and the K-split body of
// csrc/convnet_w24k.hip): the layers of 128 output channels of k_cyl_net_wg (csrc/convnet_wg.hip) in the Winograd
// F(2x4, 3x3) domain: tiles of 2 rows x 4 azimuth columns (20 = 5 x 4), a 4 x 6 input window, 4 x 6 = 24 components,
//     Y = A2^T [ sum_c (G2 g G4^T)[c] (.) (B2^T d[c] B4) ] A4           (F(2,3) down the rows as before, F(4,3) along the azimuth:
//                                                                         the points 0, +-1, +-2, infinity)
// One M-tile carries the map: lanes 0..14 hold tile (ty = li / 5, tx = li % 5) of the output rows 0..5, lane 15 the tile whose window
// is rows 5, 6 and two padding rows at columns 15..20 and which produces row 6, columns 16..19 (its second output row does not
// exist and is dropped).  Row 6, columns 0..15 stays in the direct form.  24 + 6 = 30 matrix instructions per (4 input, 16 output
// channels) against the 38 of the F(2x2) form.  The other layer forms (64 and 32 output channels) are those of k_cyl_net_wg: one
// Winograd M-tile would leave their wavefronts one N-tile each.
//
// Opt-in: bit 1 of relu_host[l] (WG_F24_FLAG) says that layer l's filter buffer holds the F(2x4) set (buf_winograd_f24_tile_weights,
// 24 Cout Cin floats) BEHIND the F(2x2) set; the stack runs here if any layer carries it (cyl_kernel_for, csrc/cnn_launch.hip).  Every layer of 128 output channels must
// carry it then, and no other layer may.
//
// The pair form: wavefront w owns the N-tile pair 2w, 2w+1 over the whole K.  Four passes over the row components; per k-step a pass
// reads two window rows of six words (three ds_read_b64 each: the window starts at the even word 4 tx of the row layout), forms the
// six row combinations and the six column components (18 plain or fused instructions) and issues 12 MFMAs back to back -- 1.5
// vector instructions per MFMA.  Same three-stage software pipeline and fences as wg_pass.
//
// Filter tiling [pair][i][k-step][ n2: [lk][li][j = 0, 1, 2, 5] | n2: [lk][li][j = 3, 4] ]: a lane's six components of a block row
// are a 16-byte and an 8-byte buffer load, and the 16-byte part is all the direct round needs: its taps are
//     g[a][0] = 4 U_a0,    g[a][1] = -3 (U_a1 - U_a2),    g[a][2] = U_a5        (row components U_0 for a = 0, U_1 - U_2 for a = 1)
// and the factors 4, -3, 1 are applied ONCE, to one accumulator per azimuth tap.
#include "common.h"

#define W24_WSTRIDE 768        // floats per (row component, k-step) of an N-tile pair: 2 x 256 + 2 x 128
#define W24_SET_F22(CIN) (16 * 128 * (CIN))     // floats of the F(2x2) set in front of the F(2x4) set (128 output channels)

// tile (ty, tx) of lane column li
__device__ __forceinline__ void w24_tile(int li, int& ty, int& tx)
{
    const bool last = li == 15;
    ty = last ? 3 : li / 5;
    tx = last ? 4 : li - 5 * ty;
}

// LDS byte address of window row a (0..3) of the lane's tile, for the lane's channel of k-step 0: six words from the halo word
// of column 4 tx - 1 on.  A row outside the map reads the channel's four zeros and its two dump words, which the layer zeroes first.
__device__ __forceinline__ unsigned w24_row_addr(unsigned act_addr, int a, int li, int lk)
{
    int ty, tx;
    w24_tile(li, ty, tx);
    const int row = 2 * ty - 1 + a;
    return act_addr + 4u * (unsigned)(lk * WG_CS + ((row >= 0 && row <= 6) ? row * WG_ROW + 4 * tx : WG_ZERO));
}

struct W24AddrPark { float a[4]; };
__device__ __forceinline__ void w24_park_addresses(const float* act, int li, int lk, W24AddrPark& pk)
{
    const unsigned act_addr = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)act;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const unsigned v = w24_row_addr(act_addr, a, li, lk);
        asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(pk.a[a]) : "v"(v));
    }
}

// Two window rows of six words.  Three ds_read_b64 per row: the empty asm keeps them from being fused into ds_read2_b64.
#define W24_LOAD(DST, A0, A1_, OFS)                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int q_ = 0; q_ < 3; q_++) {                                                \
            DST[q_] = *(wg_lds_f2)(size_t)((A0) + (OFS) + 8 * q_);                                        \
            asm volatile("" : "+v"(A0));                                                                  \
        }                                                                                                 \
        _Pragma("unroll") for (int q_ = 0; q_ < 3; q_++) {                                                \
            DST[3 + q_] = *(wg_lds_f2)(size_t)((A1_) + (OFS) + 8 * q_);                                   \
            asm volatile("" : "+v"(A1_));                                                                 \
        }                                                                                                 \
    }

__device__ __forceinline__ wgf2 w24_ldw2(__amdgpu_buffer_rsrc_t rs, unsigned uniform_float_ofs, unsigned lane_byte_ofs)
{
    return __builtin_bit_cast(wgf2, __builtin_amdgcn_raw_buffer_load_b64(rs, lane_byte_ofs, uniform_float_ofs * 4, 0));
}

// component j = 0..5 of N-tile n's block row in ring slot k
#define W24_U(n, k, j) ((j) < 3 ? W4[n][k][j] : ((j) == 5 ? W4[n][k][3] : W2[n][k][(j) - 3]))

// One row component I over `niter` x 4 k-steps for the N-tile pair: acc[n][j] += V_Ij(tile, c) * U_Ij(c, n).  The structure is
// wg_pass's with one M-tile: step s issues the LDS reads of step s + 2, runs the 12 MFMAs of step s, then forms the operands of
// step s + 1; the weights (a ring of two k-steps) are reloaded with the k-step two further on as soon as their MFMAs are through.
template <int I, bool PRIMED, int INEXT, unsigned KSTEP = WG_KSTEP>
__device__ __forceinline__ void w24_pass(unsigned (&RA)[4], __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned wp_next, unsigned lofs4, unsigned lofs2,
                                         int niter, wgf4 (&W4)[2][2], wgf2 (&W2)[2][2], wgf4 (&acc)[2][6], wgf2 (&D)[2][6])
{
    constexpr int A1 = wg_a1(I), A2 = wg_a2(I);
    constexpr int A1N = wg_a1(INEXT < 0 ? 0 : INEXT), A2N = wg_a2(INEXT < 0 ? 0 : INEXT);
    float V[2][6];
    unsigned P0 = RA[A1], P1 = RA[A2];
    if constexpr (!PRIMED) {
        W24_LOAD(D[0], P0, P1, 0)
        W24_LOAD(D[1], P0, P1, KSTEP)
    }
    // row component (d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3) of the six words, then B4^T:
    //     t0 = 4 r0 - 5 r2 + r4,   t1,2 = (r4 - 4 r2) +- (r3 - 4 r1),   t3,4 = (r4 - r2) +- 2 (r3 - r1),   t5 = 4 r1 - 5 r3 + r5
#define W24_XFORM(BUF)                                                                                    \
    {                                                                                                     \
        float r_[6];                                                                                      \
        _Pragma("unroll") for (int b = 0; b < 6; b++) {                                                   \
            const float da_ = D[BUF][b >> 1][b & 1];                                                      \
            const float db_ = D[BUF][3 + (b >> 1)][b & 1];                                                \
            r_[b] = I == 1 ? wg_add(da_, db_) : (I == 2 ? wg_sub(db_, da_) : wg_sub(da_, db_));           \
        }                                                                                                 \
        const float c_ = wg_sub(r_[4], r_[2]), e_ = wg_sub(r_[3], r_[1]);                                 \
        const float a_ = __builtin_fmaf(-4.f, r_[2], r_[4]), b_ = __builtin_fmaf(-4.f, r_[1], r_[3]);     \
        V[BUF][0] = __builtin_fmaf(4.f, r_[0], __builtin_fmaf(-4.f, r_[2], c_));                          \
        V[BUF][1] = wg_add(a_, b_); V[BUF][2] = wg_sub(a_, b_);                                           \
        V[BUF][3] = __builtin_fmaf(2.f, e_, c_); V[BUF][4] = __builtin_fmaf(-2.f, e_, c_);                \
        V[BUF][5] = __builtin_fmaf(-4.f, e_, wg_sub(r_[5], r_[3]));                                       \
    }
    W24_XFORM(0)
#pragma unroll 1
    for (int it = 0; it < niter; it++) {
        const bool more = it + 1 < niter;
        const unsigned wcur = wp + 4 * it * W24_WSTRIDE;          // this iteration's k-steps 2, 3 ...
        const unsigned wn = more ? wcur + 4 * W24_WSTRIDE : wp_next;   // ... and the k-steps 0, 1 of the next one (or of the next pass)
        const unsigned adv = more ? 4u * KSTEP : 0u;           // past the end: the iteration's own first steps again (unused)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (s < 2) W24_LOAD(D[s & 1], P0, P1, (s + 2) * KSTEP)
            else {
                if (s == 2) { P0 += adv; P1 += adv; }              // the next iteration's base from here on
                if constexpr (INEXT >= 0) {                        // last iteration: the next pass's first steps instead
                    unsigned q0 = more ? P0 : RA[A1N], q1 = more ? P1 : RA[A2N];
                    W24_LOAD(D[s & 1], q0, q1, (s - 2) * KSTEP)
                } else
                    W24_LOAD(D[s & 1], P0, P1, (s - 2) * KSTEP)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < 2; n++)
#pragma unroll
                for (int j = 0; j < 6; j++)
                    acc[n][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(W24_U(n, s & 1, j), V[s & 1][j], acc[n][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            W24_XFORM((s + 1) & 1)
#pragma unroll
            for (int n = 0; n < 2; n++) {                          // k-step s is through: its registers take the k-step two further on
                const unsigned o = s < 2 ? wcur + (s + 2) * W24_WSTRIDE : wn + (s - 2) * W24_WSTRIDE;
                W4[n][s & 1] = wg_ldw(rs, o + n * 256, lofs4);
                W2[n][s & 1] = w24_ldw2(rs, o + 512 + n * 128, lofs2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef W24_XFORM
}

// All 24 components of the N-tile pair: Y[n][u][v] = the 2 x 4 outputs of the lane's tile.  The accumulators run on through the four
// passes as in wg_round (after pass I they hold the sum of the row components 0..I, F_I = its column transform A4^T):
//     output row 0 = F_2,      output row 1 = -F_0 + 2 F_1 - F_3
// The bias enters column component 1 -- the one A4^T carries into all four columns with weight 1 -- before pass 1.
// On entry W holds the first two k-steps at wp, on exit those at wp_after.
// NOBIAS: bias_lane may be null, as in wg_round (the upper K half of w24k_layer_ksplit, csrc/convnet_w24k.hip, carries no bias).
// KSTEP: LDS bytes between k-steps, as in wg_round (the cost net's maps, csrc/costnet_w24.hip).
template <bool NOBIAS = false, unsigned KSTEP = WG_KSTEP>
__device__ __forceinline__ void w24_round(unsigned (&RA)[4], __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned wp_after, unsigned lofs4, unsigned lofs2,
                                          int niter, unsigned pstride, const float* __restrict__ bias_lane, wgf4 (&W4)[2][2], wgf2 (&W2)[2][2],
                                          wgf4 (&Y)[2][2][4])
{
    using std::integral_constant;
    wgf2 D[2][6];
    wgf4 bv[2];
#pragma unroll
    for (int n = 0; n < 2; n++) {
        if constexpr (NOBIAS) bv[n] = bias_lane ? *reinterpret_cast<const wgf4*>(bias_lane + n * 16) : (wgf4){ 0.f, 0.f, 0.f, 0.f };
        else bv[n] = *reinterpret_cast<const wgf4*>(bias_lane + n * 16);
    }
    wgf4 acc[2][6];
    float zero = 0.f;
    asm volatile("" : "+v"(zero));                   // (an opaque zero: see wg_round)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int j = 0; j < 6; j++) acc[n][j] = (wgf4){ zero, zero, zero, zero };
    auto run = [&](auto ic) __attribute__((always_inline)) {
        constexpr int I = decltype(ic)::value;
        constexpr int INEXT = I == 3 ? 0 : I + 1;
        if constexpr (I == 1) {
#pragma unroll
            for (int n = 0; n < 2; n++) acc[n][1] += bv[n];
        }
        constexpr int ICHAIN = (INEXT != 0 && wg_chains(I)) ? INEXT : -1;
        w24_pass<I, wg_chains(I - 1), ICHAIN, KSTEP>(RA, rs, wp + I * pstride, INEXT == 0 ? wp_after : wp + (I + 1) * pstride, lofs4, lofs2, niter, W4, W2, acc, D);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 2; n++) {
            wgf4 f[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {            // A4^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1] on shared sums and differences
                const float p = acc[n][1][r] + acc[n][2][r], q = acc[n][1][r] - acc[n][2][r];
                const float t = acc[n][3][r] + acc[n][4][r], d = acc[n][3][r] - acc[n][4][r];
                f[0][r] = acc[n][0][r] + p + t;
                f[1][r] = __builtin_fmaf(2.f, d, q);
                f[2][r] = __builtin_fmaf(4.f, t, p);
                f[3][r] = __builtin_fmaf(8.f, d, q) + acc[n][5][r];
            }
#pragma unroll
            for (int v = 0; v < 4; v++) {
                if constexpr (I == 0) Y[n][1][v] = f[v];                            // F_0 (enters with a minus sign below)
                else if constexpr (I == 1) {
#pragma unroll
                    for (int r = 0; r < 4; r++) Y[n][1][v][r] = __builtin_fmaf(2.f, f[v][r], -Y[n][1][v][r]);
                }
                else if constexpr (I == 2) Y[n][0][v] = f[v];
                else Y[n][1][v] -= f[v];
                // pinned here, as in wg_round: left free the sums sink below the next pass's loop and the accumulators are carried instead
                if constexpr (I == 2) asm volatile("" : "+v"(Y[n][0][v]));
                else asm volatile("" : "+v"(Y[n][1][v]));
            }
        }
    };
    run(integral_constant<int, 0>{});
    run(integral_constant<int, 1>{});
    run(integral_constant<int, 2>{});
    run(integral_constant<int, 3>{});
}

// Output row 6, columns 0..15 of the N-tile pair in the direct form: wg_round_direct's steps and pipeline on the 16-byte parts of the
// F(2x4) block rows 0..2.  One accumulator per AZIMUTH tap b (the filter rows a = 0, 1 add up in it, K ascending): the taps as formed
// from the blocks are g[a][b] / (4, -3, 1)[b], and y = 4 acc_0 - 3 acc_1 + acc_2 once at the end; the bias starts in acc_2.
// On entry W4 holds block 0's first two k-steps.  NOBIAS: bias_lane may be null.
template <bool NOBIAS = false>
__device__ __forceinline__ void w24_round_direct(unsigned row5, __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned lofs, int niter, unsigned pstride,
                                                 const float* __restrict__ bias_lane, wgf4 (&W4)[2][2], wgf4 (&Y)[2])
{
    constexpr int wstride = W24_WSTRIDE;
    wgf4 Wr[3][2][2];                                           // blocks 0..2, N-tile, two k-steps each
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            Wr[0][n][k] = W4[n][k];
            Wr[1][n][k] = wg_ldw(rs, wp + pstride + n * 256 + k * wstride, lofs);
            Wr[2][n][k] = wg_ldw(rs, wp + 2 * pstride + n * 256 + k * wstride, lofs);
        }
    float X[2][6];                                              // window words [row 5 | row 6][tap] of two steps in flight
    unsigned pa = row5;
    WG_LOADD(X[0], pa, 0)
    WG_LOADD(X[1], pa, WG_KSTEP)
    wgf4 acc[2][3];
    float zero = 0.f;
    asm volatile("" : "+v"(zero));
#pragma unroll
    for (int n = 0; n < 2; n++) {
        acc[n][0] = (wgf4){ zero, zero, zero, zero };
        acc[n][1] = (wgf4){ zero, zero, zero, zero };
        if constexpr (NOBIAS) acc[n][2] = bias_lane ? *reinterpret_cast<const wgf4*>(bias_lane + n * 16) : (wgf4){ zero, zero, zero, zero };
        else acc[n][2] = *reinterpret_cast<const wgf4*>(bias_lane + n * 16);
    }
    float G[2][6];
#define W24_TAPS(SLOT)                                                                                    \
    _Pragma("unroll") for (int n = 0; n < 2; n++) {                                                       \
        const wgf4 u0_ = Wr[0][n][SLOT], u1_ = Wr[1][n][SLOT], u2_ = Wr[2][n][SLOT];                      \
        const float d1_ = wg_sub(u1_[1], u2_[1]), d2_ = wg_sub(u1_[2], u2_[2]);                           \
        G[n][0] = u0_[0]; G[n][1] = wg_sub(u0_[1], u0_[2]); G[n][2] = u0_[3];                             \
        G[n][3] = wg_sub(u1_[0], u2_[0]); G[n][4] = wg_sub(d1_, d2_); G[n][5] = wg_sub(u1_[3], u2_[3]);   \
    }
#define W24_RELOAD(SLOT, OFS)                                                                             \
    _Pragma("unroll") for (int n = 0; n < 2; n++)                                                         \
        _Pragma("unroll") for (int blk = 0; blk < 3; blk++) Wr[blk][n][SLOT] = wg_ldw(rs, (OFS) + blk * pstride + n * 256, lofs);
    W24_TAPS(0)
    W24_RELOAD(0, wp + 2 * wstride)
#pragma unroll 1
    for (int it = 0; it < niter; it++) {
        const bool more = it + 1 < niter;
        const unsigned wcur = wp + 4 * it * wstride;
        const unsigned wn = more ? wcur + 4 * wstride : wp;      // past the end: the round's own first k-steps again (unused, in bounds)
        const unsigned adv = more ? 4u * WG_KSTEP : 0u;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++) {
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int n = 0; n < 2; n++)
                        acc[n][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(G[n][a * 3 + b], X[s & 1][a * 3 + b], acc[n][b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (s < 2) WG_LOADD(X[s & 1], pa, (s + 2) * WG_KSTEP)
            else {
                if (s == 2) pa += adv;                           // the next iteration's base from here on
                WG_LOADD(X[s & 1], pa, (s - 2) * WG_KSTEP)
            }
            __builtin_amdgcn_sched_barrier(0);
            W24_TAPS((s + 1) & 1)                                // k-step s + 1's taps; its registers take the k-step two further on
            if (s == 0) W24_RELOAD(1, wcur + 3 * wstride)
            else W24_RELOAD((s + 1) & 1, wn + (s - 1) * wstride)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef W24_TAPS
#undef W24_RELOAD
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 4; r++) Y[n][r] = __builtin_fmaf(4.f, acc[n][0][r], __builtin_fmaf(-3.f, acc[n][1][r], acc[n][2][r]));
}

// ReLU + store of one N-tile's 2 x 4 tiles into the activation buffer with the circular halo copies (C/D layout: lane column li = the
// tile, rows lk * 4 + r = the output channel).  Straight-line code as in wg_store_tile: what a lane has no place for (lane 15's second
// row, the halo copies of the inner tiles) goes to the channel's two dump words.
__device__ __forceinline__ void w24_store_tile(const wgf4 (&Yt)[2][4], int nt, int relu, float* __restrict__ act, int li, int lk)
{
    const int n0 = nt * 16 + lk * 4;
    const float lo = relu ? 0.f : -__builtin_inff();
    int ty, tx;
    w24_tile(li, ty, tx);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int row = 2 * ty + u;
        const bool ok = row < 7;
        int pos[4];
#pragma unroll
        for (int v = 0; v < 4; v++) pos[v] = ok ? row * WG_ROW + 4 * tx + 1 + v : WG_ZERO + 4;
        const int h0 = (ok && tx == 0) ? row * WG_ROW + 21 : WG_ZERO + 4;      // column 0 again behind column 19
        const int h1 = (ok && tx == 4) ? row * WG_ROW : WG_ZERO + 5;           // column 19 again in front of column 0
        float* p = act + n0 * WG_CS;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float val[4];
#pragma unroll
            for (int v = 0; v < 4; v++) { val[v] = fmaxf(Yt[u][v][r], lo); p[r * WG_CS + pos[v]] = val[v]; }
            p[r * WG_CS + h0] = val[0]; p[r * WG_CS + h1] = val[3];
        }
    }
}

// One layer with 128 output channels in the F(2x4) form: wavefront `pair` owns the N-tiles 2 pair, 2 pair + 1 over the whole K.  The
// held outputs (64 of the Winograd round, then 8 of row 6) wait for the in-place barrier in accumulation registers, as in wg_layer_pair.
// wt: the layer's F(2x4) set.
__device__ __forceinline__ void w24_layer_pair(float* __restrict__ act, const float* __restrict__ wt, const float* __restrict__ bias, int cin, int relu,
                                               int pair, const WgAddrPark& pk, const W24AddrPark& pk24)
{
    // A window row in the elevation padding is six words from the channel's zero area on: its four zeros and its two dump words, which
    // the stores of the previous layer (or nobody yet) have written.  Zeroed here, one word per thread; the layer's own stores come
    // after its in-place barrier.
    act[(threadIdx.x >> 1) * WG_CS + WG_ZERO + 4 + (threadIdx.x & 1)] = 0.f;
    __syncthreads();
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int k4 = cin >> 2;
    unsigned RA[4];
#pragma unroll
    for (int a = 0; a < 4; a++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(RA[a]) : "a"(pk24.a[a]));
    const unsigned row5 = wg_parked(pk, 2, 0);
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned pstride = (unsigned)(k4 * W24_WSTRIDE);
    const unsigned wp = (unsigned)pair * 4 * pstride;                      // [pair][i][k-step][...]
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    const float* bv = bias + (2 * pair) * 16 + lk * 4;
    wgf4 W4[2][2];
    wgf2 W2[2][2];
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            W4[n][k] = wg_ldw(rs, wp + k * W24_WSTRIDE + n * 256, lofs4);
            W2[n][k] = w24_ldw2(rs, wp + k * W24_WSTRIDE + 512 + n * 128, lofs2);
        }
    wgf4 Y[2][2][4];
    float park[2][36];
    w24_round(RA, rs, wp, wp, lofs4, lofs2, k4 >> 2, pstride, bv, W4, W2, Y);
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int q = 0; q < 32; q++) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][q]) : "v"(Y[n][q >> 4][(q >> 2) & 3][q & 3]));
    wgf4 Yb[2];
    w24_round_direct(row5, rs, wp, lofs4, k4 >> 2, pstride, bv, W4, Yb);
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int q = 0; q < 4; q++) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][32 + q]) : "v"(Yb[n][q]));
    __syncthreads();                                 // every wavefront has finished reading the layer's input
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the store offsets are formed here, not kept from the layer's start
#pragma unroll
    for (int n = 0; n < 2; n++) {
#pragma unroll
        for (int q = 0; q < 32; q++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(Y[n][q >> 4][(q >> 2) & 3][q & 3]) : "a"(park[n][q]));
#pragma unroll
        for (int q = 0; q < 4; q++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(Yb[n][q]) : "a"(park[n][32 + q]));
        w24_store_tile(Y[n], 2 * pair + n, relu, act, lane_s & 15, lane_s >> 4);
        wg_store_row6<false>(Yb[n], 2 * pair + n, relu, act, nullptr, lane_s & 15, lane_s >> 4);
    }
}

// Host helper: filters w [Cout][Cin][3][3] (BN folded) -> U = G2 g G4^T in fp64, rounded once: 4 row x 6 column components in the
// tiling w24_layer_pair streams,
//     out[24 * Cout * Cin] = [pair][i][k-step][ n2: [lk][li][q] | n2: [lk][li][j - 3] ]
// with q = 0..3 the column components j = 0, 1, 2, 5 (2 x 256 floats) and then j = 3, 4 (2 x 128 floats) of
// U[i][j][16 (2 pair + n2) + li][4 ks + lk].  No device work.
extern "C" int buf_winograd_f24_tile_weights(const float* w_host, int cout, int cin, float* out_host)
{
    BUF_REQUIRE(w_host && out_host, BUF_EINVAL, "buf_winograd_f24_tile_weights: null argument");
    BUF_REQUIRE(cout > 0 && cin > 0 && cout % 32 == 0 && cin % 4 == 0, BUF_EINVAL, "buf_winograd_f24_tile_weights: widths %d -> %d", cin, cout);
    static const double G2[4][3] = { { 1, 0, 0 }, { .5, .5, .5 }, { .5, -.5, .5 }, { 0, 0, 1 } };
    const double s6 = 1.0 / 6, s12 = 1.0 / 12, s24 = 1.0 / 24;
    const double G4[6][3] = { { .25, 0, 0 }, { -s6, -s6, -s6 }, { -s6, s6, -s6 }, { s24, s12, s6 }, { s24, -s12, s6 }, { 0, 0, 1 } };
    const int k4 = cin / 4;
    for (int o = 0; o < cout; o++)
        for (int c = 0; c < cin; c++) {
            const float* g = w_host + ((size_t)o * cin + c) * 9;
            const int n = o / 16, lane = (c % 4) * 16 + o % 16;
            for (int i = 0; i < 4; i++) {
                float* blk = out_host + (((size_t)(n / 2) * 4 + i) * k4 + c / 4) * W24_WSTRIDE;
                for (int j = 0; j < 6; j++) {
                    double u = 0;
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) u += G2[i][a] * (double)g[3 * a + b] * G4[j][b];
                    if (j == 3 || j == 4) blk[512 + (n % 2) * 128 + lane * 2 + (j - 3)] = (float)u;
                    else blk[(n % 2) * 256 + lane * 4 + (j == 5 ? 3 : j)] = (float)u;
                }
            }
        }
    return BUF_OK;
}
