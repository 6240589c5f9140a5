// A11 dense part -- w24p_layer_psplit, a layer form of the fused kernel (cyl_net_w25t_body, csrc/convnet_w25t.hip): the flagged
// 64-output layers of k_cyl_net_w24k (csrc/convnet_w24k.hip) in the "pass split" form.
// The same layers (64 output channels, Cin % 64 == 0, bit 2 of the relu word), the same filter buffers, the same 24 + 6 matrix
// instructions per (k-step, N-tile) -- 22 848 per patch of the released stack -- but split over the four wavefronts by ROW COMPONENT
// instead of by K half:
//
//   Winograd round   wavefront w owns row component I = w of the F(2,3) row transform (d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3) for ALL four
//                    N-tiles over the WHOLE K: one pass, per k-step two window rows (six ds_read_b64), one transform of 18
//                    instructions, 6 x 4 = 24 MFMAs into 96 accumulators.  No transform is formed twice in the workgroup (the K split
//                    forms each one in both wavefronts of a K half).  The filters are the blocks (pair 0, I) and (pair 1, I) of
//                    [pair][i][k-step][768], streamed at two wavefront-uniform offsets.
//   fold             A4^T once per N-tile after the loop: f_I = 4 columns x wgf4 per N-tile, 64 floats per lane (the K split folds both
//                    N-tiles of a pair after each of its four passes, in both K halves).
//   direct round     row 6, columns 0..15 of N-tile w over the whole K, the one-N-tile form of w24_round_direct; nothing exchanged.
//                    (It runs in front of the Winograd round: four held values instead of 64.)
//   finishing        wavefront q finishes N-tile q:  row 0 = (f_0 + f_1) + f_2,  row 1 = (f_1 - f_2) - f_3  (A2^T of F(2,3)); the bias
//                    rides in column component 1 of the pass of I = 1, which A4^T carries into all four columns and A2^T into both
//                    rows with weight 1.  Each wavefront gives 3 x 16 floats per lane and receives 3 x 16 through LDS.
//
// One loop body serves the four row components: the row combination is ONE v_fma per word, da + sgn db with the wavefront-uniform
// sgn = +-1 (exact: the same value as the add or subtract of w24_pass), and the two row addresses are picked per wavefront --
// (0, 2) (1, 2) (2, 1) (1, 3).  Four instantiations under a wavefront-uniform branch would issue the same instructions per wavefront
// from four times the code.
//
// The exchange area.  48 floats per lane and wavefront are 48 KB; the area of the K split (channels 64..127, words 0..143: 36.9 KB) does
// not hold that, but behind the barrier that says every wavefront has read the layer's input the whole buffer is free:
//   * 36 floats per lane in the K split's area: wavefront w writes the 16 rows from channel 64 + 16 w on, lane (row = lane >> 2,
//     quarter = lane & 3) nine float4 from word 36 quarter on -- three per receiver, receivers in ascending order;
//   * 12 floats per lane in the RECEIVERS' own output rows: the fourth float4 for receiver q goes to channel 16 q + (lane >> 2),
//     words 12 quarter + 4 s (s: the sender's rank among q's three senders).  Only q overwrites these rows, with its own stores, after
//     it has read them: no third barrier.
// Words WG_ZERO..WG_ZERO + 3 and the two dump words of every channel are not touched (layer 3 reads the zero words of the channels
// 64..127 after layer 1 has used those rows).  Barriers per flagged layer, beside the one behind the dump-word clear and the one that
// closes every layer: two at either Cin (input read | exchange in place) -- the K split has one at Cin = 64 and two at Cin = 128.
#include "common.h"

#define W24P_XCH_C 64          // first channel row of the wide part of the exchange area
#define W24P_XCH_WIDE 36       // words per lane there (nine float4)
#define W24P_XCH_OWN 12        // words per lane in a receiver's own rows (three float4, one per sender)

// The 96 accumulators of the pass live in ACCUMULATION registers.  The compiler splits the 256 registers of a kernel that parks anything
// in accumulation registers (the window addresses, the other layer forms' held outputs) 128 + 128, and 96 + 48 (filter ring) + 36 (window
// words, operands) do not fit the vector half; it is also told to keep its own matrix instructions on vector registers
// (buffer_amd/build.py), so these are written out.  An accumulator is used once per k-step, 24 matrix instructions apart, and taken whole
// as C by the next one (no wait states).  What the compiler does not pad for a statement it cannot see into: the two wait states between a
// vector instruction that wrote an operand and the first matrix instruction of a k-step (the s_nop in front of it; in the loop a dozen
// loads stand between anyway), and the states between the last matrix instruction and the first read of its result (w24p_pass ends with
// them).
#define W24P_MFMA(PRE, ACC, A, B) asm volatile(PRE "v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(ACC) : "v"(A), "v"(B));

// Row component da + sgn db of the six window words in D (one v_fma per word), then B4^T as in w24_pass, into V[BUF]; uses the caller's
// D, V and sgn.  Shared with w24a_pass (csrc/convnet_w24a.hip).
#define W24P_XFORM(BUF)                                                                                   \
    {                                                                                                     \
        float r_[6];                                                                                      \
        _Pragma("unroll") for (int b = 0; b < 6; b++)                                                     \
            r_[b] = __builtin_fmaf(sgn, D[3 + (b >> 1)][b & 1], D[b >> 1][b & 1]);                       \
        const float c_ = wg_sub(r_[4], r_[2]), e_ = wg_sub(r_[3], r_[1]);                                 \
        const float a_ = __builtin_fmaf(-4.f, r_[2], r_[4]), b_ = __builtin_fmaf(-4.f, r_[1], r_[3]);     \
        V[BUF][0] = __builtin_fmaf(4.f, r_[0], __builtin_fmaf(-4.f, r_[2], c_));                          \
        V[BUF][1] = wg_add(a_, b_); V[BUF][2] = wg_sub(a_, b_);                                           \
        V[BUF][3] = __builtin_fmaf(2.f, e_, c_); V[BUF][4] = __builtin_fmaf(-2.f, e_, c_);                \
        V[BUF][5] = __builtin_fmaf(-4.f, e_, wg_sub(r_[5], r_[3]));                                       \
    }

// Row component `I = w` over `niter` x 4 k-steps for all four N-tiles: acc[n][j] += V_Ij(tile, c) * U_Ij(c, n).  w24_pass's steps and
// fences with four N-tiles behind one transform and the LDS reads ONE step ahead (step s reads the words of step s + 1, runs its
// 24 MFMAs, then forms the operands of step s + 1); P0 / P1: the two window rows (da, db), sgn: the sign of db.
// On entry W holds the first two k-steps of the blocks at wp0 (N-tiles 0, 1) and wp1 (N-tiles 2, 3); the last iteration fetches the
// k-steps 0, 1 at wp_next into every ring slot instead (unused by the pass-split layer, in bounds).
__device__ __forceinline__ void w24p_pass(unsigned P0, unsigned P1, float sgn, __amdgpu_buffer_rsrc_t rs, unsigned wp0, unsigned wp1, unsigned wp_next,
                                          unsigned lofs4, unsigned lofs2, int niter, wgf4 (&W4)[4][2], wgf2 (&W2)[4][2], wgf4 (&acc)[4][6])
{
    wgf2 D[6];                                       // one k-step of window words in flight: a k-step is 24 matrix instructions long
    float V[2][6];
    W24_LOAD(D, P0, P1, 0)
    W24P_XFORM(0)
    int it = 0;
#pragma unroll 1
    do {                                             // (niter >= 1: a loop that may run zero times keeps a second copy of the accumulators' start)
        const bool more = it + 1 < niter;
        const unsigned wcur0 = wp0 + 4 * it * W24_WSTRIDE, wcur1 = wp1 + 4 * it * W24_WSTRIDE;     // this iteration's k-steps 2, 3 ...
        const unsigned wn0 = more ? wcur0 + 4 * W24_WSTRIDE : wp_next;                             // ... and the k-steps 0, 1 of the next one
        const unsigned wn1 = more ? wcur1 + 4 * W24_WSTRIDE : wp_next;
        const unsigned adv = more ? 4u * WG_KSTEP : 0u;           // past the end: the iteration's own first steps again (unused)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (s < 3) W24_LOAD(D, P0, P1, (s + 1) * WG_KSTEP)
            else {
                P0 += adv; P1 += adv;                              // the next iteration's base
                W24_LOAD(D, P0, P1, 0)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < 4; n++)
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    if (n == 0 && j == 0) W24P_MFMA("s_nop 1\n\t", acc[n][j], W24_U(n, s & 1, j), V[s & 1][j])
                    else W24P_MFMA("", acc[n][j], W24_U(n, s & 1, j), V[s & 1][j])
                }
            __builtin_amdgcn_sched_barrier(0);
            W24P_XFORM((s + 1) & 1)
#pragma unroll
            for (int n = 0; n < 4; n++) {                          // k-step s is through: its registers take the k-step two further on
                const unsigned o = n < 2 ? (s < 2 ? wcur0 + (s + 2) * W24_WSTRIDE : wn0 + (s - 2) * W24_WSTRIDE)
                                         : (s < 2 ? wcur1 + (s + 2) * W24_WSTRIDE : wn1 + (s - 2) * W24_WSTRIDE);
                W4[n][s & 1] = wg_ldw(rs, o + (n & 1) * 256, lofs4);
                W2[n][s & 1] = w24_ldw2(rs, o + 512 + (n & 1) * 128, lofs2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } while (++it < niter);
    // The last matrix instructions' results (8 passes each) before anything reads them: the operands make every read wait for this
    // statement.  (In the loop the transform and the reloads of a step stand behind its matrix instructions as well.)
    asm volatile("s_nop 15"
                 : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+a"(acc[0][5]), "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[1][4]), "+a"(acc[1][5]), "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]), "+a"(acc[2][4]), "+a"(acc[2][5]), "+a"(acc[3][0]), "+a"(acc[3][1]), "+a"(acc[3][2]), "+a"(acc[3][3]), "+a"(acc[3][4]), "+a"(acc[3][5]));
}

// Output row 6, columns 0..15 of ONE N-tile in the direct form: w24_round_direct's steps, pipeline and summation order (one
// accumulator per azimuth tap, the filter rows a = 0, 1 add up in it, K ascending; y = 4 acc_0 - 3 acc_1 + acc_2, the bias starts in
// acc_2).  The six MFMAs of a k-step go round the three accumulators twice, so none waits for its predecessor.
// wp: block 0 of the N-tile's pair plus 256 n2; W0: its first two k-steps.  NOBIAS: bias_lane may be null (the upper K half of
// w24a_layer_psplit32, csrc/convnet_w24a.hip, carries no bias).
template <bool NOBIAS = false>
__device__ __forceinline__ void w24p_round_direct(unsigned row5, __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned lofs, int niter, unsigned pstride,
                                                  const float* __restrict__ bias_lane, const wgf4 (&W0)[2], wgf4& Y)
{
    constexpr int wstride = W24_WSTRIDE;
    wgf4 Wr[3][2];                                              // blocks 0..2, two k-steps each
#pragma unroll
    for (int k = 0; k < 2; k++) {
        Wr[0][k] = W0[k];
        Wr[1][k] = wg_ldw(rs, wp + pstride + k * wstride, lofs);
        Wr[2][k] = wg_ldw(rs, wp + 2 * pstride + k * wstride, lofs);
    }
    float X[2][6];                                              // window words [row 5 | row 6][tap] of two steps in flight
    unsigned pa = row5;
    WG_LOADD(X[0], pa, 0)
    WG_LOADD(X[1], pa, WG_KSTEP)
    wgf4 acc[3];
    float zero = 0.f;
    asm volatile("" : "+v"(zero));
    acc[0] = (wgf4){ zero, zero, zero, zero };
    acc[1] = (wgf4){ zero, zero, zero, zero };
    if constexpr (NOBIAS) acc[2] = bias_lane ? *reinterpret_cast<const wgf4*>(bias_lane) : (wgf4){ zero, zero, zero, zero };
    else acc[2] = *reinterpret_cast<const wgf4*>(bias_lane);
    float G[6];
#define W24P_TAPS(SLOT)                                                                                   \
    {                                                                                                     \
        const wgf4 u0_ = Wr[0][SLOT], u1_ = Wr[1][SLOT], u2_ = Wr[2][SLOT];                               \
        const float d1_ = wg_sub(u1_[1], u2_[1]), d2_ = wg_sub(u1_[2], u2_[2]);                           \
        G[0] = u0_[0]; G[1] = wg_sub(u0_[1], u0_[2]); G[2] = u0_[3];                                      \
        G[3] = wg_sub(u1_[0], u2_[0]); G[4] = wg_sub(d1_, d2_); G[5] = wg_sub(u1_[3], u2_[3]);            \
    }
#define W24P_RELOAD(SLOT, OFS)                                                                            \
    _Pragma("unroll") for (int blk = 0; blk < 3; blk++) Wr[blk][SLOT] = wg_ldw(rs, (OFS) + blk * pstride, lofs);
    W24P_TAPS(0)
    W24P_RELOAD(0, wp + 2 * wstride)
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
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 3; b++)
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(G[a * 3 + b], X[s & 1][a * 3 + b], acc[b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (s < 2) WG_LOADD(X[s & 1], pa, (s + 2) * WG_KSTEP)
            else {
                if (s == 2) pa += adv;                           // the next iteration's base from here on
                WG_LOADD(X[s & 1], pa, (s - 2) * WG_KSTEP)
            }
            __builtin_amdgcn_sched_barrier(0);
            W24P_TAPS((s + 1) & 1)                               // k-step s + 1's taps; its registers take the k-step two further on
            if (s == 0) W24P_RELOAD(1, wcur + 3 * wstride)
            else W24P_RELOAD((s + 1) & 1, wn + (s - 1) * wstride)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef W24P_TAPS
#undef W24P_RELOAD
#pragma unroll
    for (int r = 0; r < 4; r++) Y[r] = __builtin_fmaf(4.f, acc[0][r], __builtin_fmaf(-3.f, acc[1][r], acc[2][r]));
}

// Wavefront W hands f_W of the N-tiles q != W to their finishers: three float4 to its own rows of the wide area, the fourth to q's rows
template <int W>
__device__ __forceinline__ void w24p_give(const wgf4 (&f)[4][4], float* __restrict__ act, int lane)
{
    float* wide = act + (W24P_XCH_C + 16 * W + (lane >> 2)) * WG_CS + (lane & 3) * W24P_XCH_WIDE;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (q == W) continue;
        const int slot = q - (q > W), rank = W - (W > q);         // q among W's receivers, W among q's senders
#pragma unroll
        for (int v = 0; v < 3; v++) *reinterpret_cast<wgf4*>(wide + 12 * slot + 4 * v) = f[q][v];
        *reinterpret_cast<wgf4*>(act + (16 * q + (lane >> 2)) * WG_CS + (lane & 3) * W24P_XCH_OWN + 4 * rank) = f[q][3];
    }
}

// Wavefront Q finishes N-tile Q: its own f_Q and the three received ones, rows combined in one order for every Q
template <int Q>
__device__ __forceinline__ void w24p_take(const wgf4 (&f)[4][4], const float* __restrict__ act, int lane, wgf4 (&Yk)[2][4])
{
    const float* own = act + (16 * Q + (lane >> 2)) * WG_CS + (lane & 3) * W24P_XCH_OWN;
#pragma unroll
    for (int h = 0; h < 2; h++) {                    // two columns at a time: all four at once crowd the vector registers
        wgf4 F[4][2];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int v = 2 * h; v < 2 * h + 2; v++) {
                const int slot = Q - (Q > i), rank = i - (i > Q);
                const float* wide = act + (W24P_XCH_C + 16 * i + (lane >> 2)) * WG_CS + (lane & 3) * W24P_XCH_WIDE;
                if (i == Q) F[i][v & 1] = f[Q][v];
                else if (v < 3) F[i][v & 1] = *reinterpret_cast<const wgf4*>(wide + 12 * slot + 4 * v);
                else F[i][v & 1] = *reinterpret_cast<const wgf4*>(own + 4 * rank);
            }
#pragma unroll
        for (int v = 2 * h; v < 2 * h + 2; v++) {
            Yk[0][v] = (F[0][v & 1] + F[1][v & 1]) + F[2][v & 1];
            Yk[1][v] = (F[1][v & 1] - F[2][v & 1]) - F[3][v & 1];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

__device__ __forceinline__ void w24p_layer_psplit(float* __restrict__ act, const float* __restrict__ wt, const float* __restrict__ bias, int cin, int relu,
                                                  int w, const WgAddrPark& pk, const W24AddrPark& pk24)
{
    // (the dump words of the input channels: see w24_layer_pair)
    act[(threadIdx.x >> 1) * WG_CS + WG_ZERO + 4 + (threadIdx.x & 1)] = 0.f;
    __syncthreads();
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int k4 = cin >> 2;
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned pstride = (unsigned)(k4 * W24_WSTRIDE);
    const unsigned wp0 = (unsigned)w * pstride, wp1 = wp0 + 4 * pstride;                     // [pair][i][k-step][...]: blocks (0, w), (1, w)
    const unsigned wpd = (unsigned)(w >> 1) * 4 * pstride + (unsigned)(w & 1) * 256;         // block 0 of N-tile w's pair, its 16-byte part
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    // The direct round runs first: its one quad waits through the pass, where the 64 folded values of the pass would have to be parked
    // through the direct round.  The pass's first two k-steps of filters are asked for behind it and behind the 96 accumulator
    // writes (held through either they cost 48 vector registers that are not there), in front of the first transform.
    const wgf4 W0[2] = { wg_ldw(rs, wpd, lofs4), wg_ldw(rs, wpd + W24_WSTRIDE, lofs4) };
    wgf4 Yb;
    w24p_round_direct(wg_parked(pk, 2, 0), rs, wpd, lofs4, k4 >> 2, pstride, bias + w * 16 + lk * 4, W0, Yb);
    unsigned RA[4];
#pragma unroll
    for (int a = 0; a < 4; a++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(RA[a]) : "a"(pk24.a[a]));
    // window rows (da, db) of row component w: (0, 2) (1, 2) (2, 1) (1, 3); db enters with sgn
    const unsigned P0 = w == 0 ? RA[0] : (w == 2 ? RA[2] : RA[1]);
    const unsigned P1 = w == 3 ? RA[3] : (w == 2 ? RA[1] : RA[2]);
    const float sgn = w == 1 ? 1.f : -1.f;
    wgf4 f[4][4];                                    // f_w: [N-tile][column] after A4^T
    {
        wgf4 acc[4][6];
        float zero = 0.f;
        asm volatile("" : "+v"(zero));               // (an opaque zero: see wg_round)
#pragma unroll
        for (int n = 0; n < 4; n++)
#pragma unroll
            for (int j = 0; j < 6; j++) acc[n][j] = (wgf4){ zero, zero, zero, zero };
        if (w == 1) {                                // the bias: once, in column component 1 of row component 1
#pragma unroll
            for (int n = 0; n < 4; n++) acc[n][1] = *reinterpret_cast<const wgf4*>(bias + n * 16 + lk * 4);
        }
#pragma unroll
        for (int n = 0; n < 4; n++)
#pragma unroll
            for (int j = 0; j < 6; j++) asm volatile("" : "+a"(acc[n][j]));
        __builtin_amdgcn_sched_barrier(0);           // (the accumulators' start first: formed beside the filter ring it crowds the vector registers)
        wgf4 W4[4][2];
        wgf2 W2[4][2];
#pragma unroll
        for (int n = 0; n < 4; n++)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const unsigned o = (n < 2 ? wp0 : wp1) + k * W24_WSTRIDE;
                W4[n][k] = wg_ldw(rs, o + (n & 1) * 256, lofs4);
                W2[n][k] = w24_ldw2(rs, o + 512 + (n & 1) * 128, lofs2);
            }
        w24p_pass(P0, P1, sgn, rs, wp0, wp1, wp0, lofs4, lofs2, k4 >> 2, W4, W2, acc);
#pragma unroll
        for (int n = 0; n < 4; n++)
#pragma unroll
            for (int r = 0; r < 4; r++) {            // A4^T as in w24_round
                const float p = acc[n][1][r] + acc[n][2][r], q = acc[n][1][r] - acc[n][2][r];
                const float t = acc[n][3][r] + acc[n][4][r], d = acc[n][3][r] - acc[n][4][r];
                f[n][0][r] = acc[n][0][r] + p + t;
                f[n][1][r] = __builtin_fmaf(2.f, d, q);
                f[n][2][r] = __builtin_fmaf(4.f, t, p);
                f[n][3][r] = __builtin_fmaf(8.f, d, q) + acc[n][5][r];
            }
    }
    __syncthreads();                                 // every wavefront has finished reading the layer's input: the whole buffer is free
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the exchange and store offsets are formed here, not kept from the layer's start
    if (w == 0) w24p_give<0>(f, act, lane_s);
    else if (w == 1) w24p_give<1>(f, act, lane_s);
    else if (w == 2) w24p_give<2>(f, act, lane_s);
    else w24p_give<3>(f, act, lane_s);
    __syncthreads();                                 // the exchange is in place
    wgf4 Yk[2][4];
    if (w == 0) w24p_take<0>(f, act, lane_s, Yk);
    else if (w == 1) w24p_take<1>(f, act, lane_s, Yk);
    else if (w == 2) w24p_take<2>(f, act, lane_s, Yk);
    else w24p_take<3>(f, act, lane_s, Yk);
    w24_store_tile(Yk, w, relu, act, lane_s & 15, lane_s >> 4);
    wg_store_row6<false>(Yb, w, relu, act, nullptr, lane_s & 15, lane_s >> 4);
}
