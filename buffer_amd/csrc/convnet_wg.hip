// A11 dense part -- Cylindrical_Net (models/patchnet.py:15-85) as ONE fused fp32-MFMA kernel in the Winograd F(2x2, 3x3)
// domain.
//
// Every layer of the stack is a 3x3 correlation over the 7 x 20 (elevation x azimuth) map (layer 0's radial depth folds
// into 48 input channels), circular in azimuth and zero-padded in elevation (utils/common.py:265-310).  With the map cut
// into 4 x 10 tiles of 2 x 2 outputs,
//     Y = A^T [ sum_c (G g G^T)[c] (.) (B^T d[c] B) ] A          (d: the tile's 4 x 4 input window)
// turns the 9-tap implicit GEMM (9 x 144 rows per channel pair) into 16 component GEMMs over tile rows.  Output row 6 (row 7
// does not exist and window rows 7, 8 are padding) runs in the DIRECT form for its columns 0..15, the M-tile that holds nothing
// else: two filter rows x three azimuth taps on 16 positions, 6 full matrix instructions (wg_round_direct).  16 + 16 + 6 = 38
// matrix instructions per (4 input, 16 output channels), 27 968 per patch of the released stack, against 75 of the direct form
// throughout.  All arithmetic stays fp32 (v_mfma_f32_16x16x4_f32); the filter transform is done
// once on the host in fp64.
//
// One workgroup owns one patch for the whole stack.  Activations live in ONE LDS buffer [128][160] (rows of 22 = 20 azimuth
// columns + the two circular halo columns, so a window row is one address + immediate offsets; 4 zeros per channel serve
// every read of the elevation padding), rewritten in place after each layer -> two workgroups per CU (2 x 80 KB).
//
// What bounds the kernel (round 3, tools/micro/mfma_group.hip): v_mfma_f32_16x16x4_f32 runs on the f32 vector lanes, so VALU
// work does NOT hide behind it -- with two waves per SIMD a matrix slot costs 32.4 + 3.6 x (VALU instructions per MFMA) cycles
// (alternating single MFMAs and VALU instructions is worse still: 52+; groups of >= 4 MFMAs are enough).  The input transform
// B^T d B costs 8 adds per 4 component operands, i.e. 2.0 VALU per MFMA if every N-tile (16 output channels) transforms for itself.
//   * 128 output channels (52 % of the MFMAs): a wavefront owns an N-tile PAIR and one transform feeds the 8 MFMAs of both
//     (1.06 VALU per MFMA in the loop).  The layer is in place -- the outputs of a pair (80 registers) wait until every
//     wavefront has read its input, in accumulation registers -- and the M-tiles run in two rounds: both Winograd tiles (64
//     accumulator registers), then row 6.
//   * 64 output channels: pairs as well, by splitting M -- a wavefront owns an N-tile pair for ONE Winograd M-tile plus row 6
//     of one N-tile (32 + 6 MFMAs per k-step for every wavefront, nothing to exchange).  32 output channels: the same inside
//     each half of K (the two wavefronts of a K split hand their partial sums over through the free upper rows of the buffer).
// The filter stream: weights come through a buffer resource with wavefront-uniform offsets (a global_load_dwordx4 with a
// 64-bit VGPR address costs ~50 cycles of SIMD issue beside MFMAs, an SGPR-based one ~10: tools/micro/mfma_vmem.hip), tiled
// so that a wavefront's k-steps are contiguous, two k-steps of weights in registers per N-tile.
// A pass walks K for one row component i of the transform: per (k-step, M-tile) step it reads two window rows (four
// ds_read_b64), forms the four column components (eight plain adds) and issues 4 MFMAs per N-tile; the accumulators run on
// through the four passes and after each pass the column transform of the running sum is folded into the 2 x 2 outputs in
// registers (the C/D layout keeps a tile in one lane).
// LDS banking (ds_read_b64: bank = word mod 64, lanes 0-31 and 32-63 served separately): the 40 tiles are dealt to the
// two Winograd M-tiles such that the 16 lanes of a k-step channel cover 32 distinct banks, and the channel stride 160 = 32 mod 64
// puts the second channel of the half-wave on the other 32:
//     M-tile 0: tile row 0 (10) + tile row 1, columns 4..9     M-tile 1: tile row 2 (10) + row 1, columns 0..3 + row 3, columns 8, 9
//     M-tile 2: output row 6, columns 0..15, one position per lane (no tiles: wg_round_direct has its own reads)
#include "common.h"
#include <type_traits>

#define WG_CS 160             // channel stride in floats: 7 x 22 + 4 zeros + 2 dump words
#define WG_ROW 22             // [col 19][col 0 .. col 19][col 0]
#define WG_ZERO 154           // zeros read by every window row outside 0 <= elevation < 7
#define WG_MAXC 128
#define WG_LAYERS 8
#define WG_THREADS 256
#define WG_BUF (WG_MAXC * WG_CS)
#define WG_KSTEP (16 * WG_CS)  // bytes between k-steps (4 channels)
#define WG_BLOCKS 16          // filter components per (input, output) channel

typedef float wgf4 __attribute__((ext_vector_type(4)));
typedef float wgf2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) wgf2* wg_lds_f2;

struct CylWgParams {
    const float* wt[WG_LAYERS];     // Winograd-domain weights, [i][k-step][N-tile][lane][j] (ops.winograd_tile_weights)
    const float* bias[WG_LAYERS];   // [Cout]
    int cin[WG_LAYERS], cout[WG_LAYERS], relu[WG_LAYERS];
    const int* only_if;             // nullable: workgroup p runs only if only_if[p] != 0 (the fp32 re-run of buf_cylindrical_net_split_safe)
    const float* taps[WG_LAYERS];   // k_cyl_net_w25t only (csrc/convnet_w25t.hip): the row-6 tap sets of the layers whose relu word says so
#ifdef WG_STAMP
    long long* stamps;              // development build (-DWG_STAMP): [workgroup][wave][20] s_memtime at the layer boundaries
#endif
};
#ifdef WG_STAMP
#define WG_STAMP_AT(SLOT) if ((threadIdx.x & 63) == 0) P.stamps[((size_t)blockIdx.x * 4 + w) * 20 + (SLOT)] = __builtin_amdgcn_s_memtime();
#else
#define WG_STAMP_AT(SLOT)
#endif

// tile (ty, tx) held by row idx of the Winograd M-tile t = 0, 1 (branch-free)
__device__ __forceinline__ bool wg_tile(int t, int idx, int& ty, int& tx)
{
    if (t == 0) { const bool a = idx < 10; ty = a ? 0 : 1; tx = a ? idx : idx - 6; return true; }
    if (t == 1) { const bool a = idx < 10, b = idx < 14; ty = a ? 2 : (b ? 1 : 3); tx = a ? idx : (b ? idx - 10 : idx - 6); return true; }
    ty = 3; tx = 0;                                            // M-tile 2 holds no tiles: output row 6 in the direct form (wg_round_direct)
    return false;
}

// LDS byte address of window row a (0..3) of the tile that lane (li, lk) holds in M-tile t, for the lane's channel of k-step 0.
// M-tile 2 is position-indexed: lane li is output column li of row 6, its window rows are 5 and 6 (a = 0, 1) from the halo word on.
__device__ __forceinline__ unsigned wg_row_addr(unsigned act_addr, int t, int a, int li, int lk)
{
    if (t == 2) return act_addr + 4u * (unsigned)(lk * WG_CS + (a < 2 ? (5 + a) * WG_ROW + li : WG_ZERO));
    int ty, tx;
    const bool ok = wg_tile(t, li, ty, tx);
    const int row = 2 * ty - 1 + a;
    return act_addr + 4u * (unsigned)(lk * WG_CS + ((ok && row >= 0 && row <= 6) ? row * WG_ROW + 2 * tx : WG_ZERO));
}

// Single adds as opaque instructions: left to itself the SLP vectoriser packs the transform into v_pk_add_f32 with a
// v_mov per operand (a packed add costs two plain ones on the issue port that the matrix pipe shares).
__device__ __forceinline__ float wg_add(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float wg_sub(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// Window rows (A1, A2) of row component I
__host__ __device__ constexpr int wg_a1(int I) { return I == 0 ? 0 : 1; }
__host__ __device__ constexpr int wg_a2(int I) { return I == 3 ? 3 : 2; }

// Does the pass of row component I hand its successor I + 1 the first two LDS steps?  (Every pass of a round has the same
// (k-step, M-tile) step shape.)
__host__ __device__ constexpr bool wg_chains(int I) { return I >= 0 && I < 3; }

// LDS reads of one step.  Two ds_read_b64 per row: the empty asm keeps the compiler from fusing them into the half-rate
// ds_read2_b64.
#define WG_LOAD2(DST, A0, A1_, OFS)                                                                       \
    {                                                                                                     \
        DST[0] = *(wg_lds_f2)(size_t)((A0) + (OFS));                                                      \
        asm volatile("" : "+v"(A0));                                                                      \
        DST[1] = *(wg_lds_f2)(size_t)((A0) + (OFS) + 8);                                                  \
        asm volatile("" : "+v"(A0));                                                                      \
        DST[2] = *(wg_lds_f2)(size_t)((A1_) + (OFS));                                                     \
        asm volatile("" : "+v"(A1_));                                                                     \
        DST[3] = *(wg_lds_f2)(size_t)((A1_) + (OFS) + 8);                                                 \
        asm volatile("" : "+v"(A1_));                                                                     \
    }


// A lane's 16 bytes of a weight block through a buffer resource: wavefront-uniform byte offset (SGPR) + the lane's 32-bit offset.
// The form matters: global_load_dwordx4 with a 64-bit VGPR address costs ~50 cycles of the SIMD's issue beside MFMAs, an
// SGPR-based address ~10 (tools/micro/mfma_vmem.hip) -- with per-lane pointers the filter stream took 8 % of the kernel.
typedef unsigned wgu4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_weights(const float* wt)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)wt, 0, 0x7fffffff, 0x00027000);
}
__device__ __forceinline__ wgf4 wg_ldw(__amdgpu_buffer_rsrc_t rs, unsigned uniform_float_ofs, unsigned lane_byte_ofs)
{
    return __builtin_bit_cast(wgf4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane_byte_ofs, uniform_float_ofs * 4, 0));
}

// One row component I of the transform over `niter` x 4 k-steps for the M-tiles [T0, T1) and NN N-tiles that share the
// transformed operand: acc[n][t][j] += V_Ij(tile, c) * U_Ij(c, n).
// The (k-step, M-tile) steps form a three-stage software pipeline held in place by sched_barriers (the compiler otherwise
// hoists the loads to the top of the loop body and waits for them at once): step s issues the LDS reads of step s+2, runs
// the 4 NN MFMAs of step s back to back, then forms the column components of step s+1.  Four k-steps per iteration: their LDS
// offsets ride in the instructions, the weights (W[n][k-step]: one 16-byte load per lane) are reloaded in place half an
// iteration ahead, and the last iteration fetches the weights of whatever runs next (wp_next) instead of its own.  Every
// pass reads its own first two steps.  The N-tiles of a pair are neighbours in the weight tiling (256 floats apart).
// KSTEP: LDS bytes between k-steps (4 channels) -- the cost net's Winograd layers run the same passes over other map sizes.
// PRIMED: the previous pass already fetched this pass's first two steps into D; INEXT >= 0: this pass fetches those of the row
// component INEXT in its last iteration (the LDS latency of a pass start is then covered by the previous pass's MFMAs).
// Weights: W[n][k-step & 1], a ring of TWO k-steps per N-tile -- the registers of a k-step are reloaded with the k-step two
// further on (of this pass, or of whatever runs next: wp_next) as soon as its MFMAs are through, so every load is issued two
// k-steps before its use with half the registers of a whole-iteration buffer (the paired layers were spilling their outputs).
template <int I, int NN, int T0, int T1, bool PRIMED, int INEXT, unsigned KSTEP = WG_KSTEP>
__device__ __forceinline__ void wg_pass(unsigned (&RA)[3][4], __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned wp_next, unsigned lofs, int niter,
                                        int wstride, wgf4 (&W)[NN][2], wgf4 (&acc)[NN][3][4], wgf2 (&D)[2][4])
{
    static_assert(T0 < T1 && T1 <= 2, "the Winograd M-tiles (M-tile 2 is wg_round_direct's)");
    constexpr int A1 = wg_a1(I), A2 = wg_a2(I);
    constexpr int NT = T1 - T0;
    constexpr int A1N = wg_a1(INEXT < 0 ? 0 : INEXT), A2N = wg_a2(INEXT < 0 ? 0 : INEXT);
    float V[2][4];
    unsigned P[NT][2];
#pragma unroll
    for (int t = 0; t < NT; t++) { P[t][0] = RA[T0 + t][A1]; P[t][1] = RA[T0 + t][A2]; }
    if constexpr (!PRIMED) {
#pragma unroll
        for (int g = 0; g < 2; g++) WG_LOAD2(D[g], P[g % NT][0], P[g % NT][1], (g / NT) * KSTEP)
    }
    // row component (d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3), then the four column components
#define WG_XFORM(BUF)                                                                                     \
    {                                                                                                     \
        float r_[4];                                                                                      \
        _Pragma("unroll") for (int b = 0; b < 4; b++) {                                                   \
            const float da_ = D[BUF][b >> 1][b & 1];                                                      \
            const float db_ = D[BUF][2 + (b >> 1)][b & 1];                                                \
            r_[b] = I == 1 ? wg_add(da_, db_) : (I == 2 ? wg_sub(db_, da_) : wg_sub(da_, db_));           \
        }                                                                                                 \
        V[BUF][0] = wg_sub(r_[0], r_[2]); V[BUF][1] = wg_add(r_[1], r_[2]);                               \
        V[BUF][2] = wg_sub(r_[2], r_[1]); V[BUF][3] = wg_sub(r_[1], r_[3]);                               \
    }
    WG_XFORM(0)
#pragma unroll 1
    for (int it = 0; it < niter; it++) {
        const bool more = it + 1 < niter;
        const unsigned wcur = wp + 4 * it * wstride;            // this iteration's k-steps 2, 3 ...
        const unsigned wn = more ? wcur + 4 * wstride : wp_next;   // ... and the k-steps 0, 1 of the next one (or of the next pass)
        const unsigned adv = more ? 4u * KSTEP : 0u;         // past the end: the iteration's own first steps again (unused)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4 * NT; s++) {
            const int t = T0 + s % NT, kk = s / NT, g = s + 2;
            if (g < 4 * NT) WG_LOAD2(D[s & 1], P[g % NT][0], P[g % NT][1], (g / NT) * KSTEP)
            else {
                const int t2 = (g - 4 * NT) % NT;                // the next iteration's base from here on (this one no longer reads through it)
                if ((g - 4 * NT) / NT == 0) { P[t2][0] += adv; P[t2][1] += adv; }
                if constexpr (INEXT >= 0) {                      // last iteration: the next pass's first steps instead
                    unsigned q0 = more ? P[t2][0] : RA[T0 + t2][A1N], q1 = more ? P[t2][1] : RA[T0 + t2][A2N];
                    WG_LOAD2(D[s & 1], q0, q1, ((g - 4 * NT) / NT) * KSTEP)
                } else
                    WG_LOAD2(D[s & 1], P[t2][0], P[t2][1], ((g - 4 * NT) / NT) * KSTEP)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < NN; n++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[n][t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(W[n][kk & 1][j], V[s & 1][j], acc[n][t][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            WG_XFORM((s + 1) & 1)
            if (s % NT == NT - 1) {                              // k-step kk is through: its registers take the k-step two further on
#pragma unroll
                for (int n = 0; n < NN; n++)
                    W[n][kk & 1] = kk < 2 ? wg_ldw(rs, wcur + n * 256 + (kk + 2) * wstride, lofs) : wg_ldw(rs, wn + n * 256 + (kk - 2) * wstride, lofs);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 2; t < NT; t++) { P[t][0] += adv; P[t][1] += adv; }     // the first two M-tiles were advanced by the look-ahead steps
    }
#undef WG_XFORM
}

// All 16 components of NN N-tiles over the M-tiles [T0, T1): Y[n][t][u][v] = 2 x 2 outputs of the tiles of M-tile t (C/D
// layout: tile = lane's column).  On entry W holds the weights of the first four k-steps; on exit those at wp_after.
// The accumulators run on through the four passes (cleared once): after pass I they hold the sum of the row components
// 0..I, F_I = its column transform, and with s_i = F_i - F_(i-1)
//     output row 0 = s_0 + s_1 + s_2 = F_2,      output row 1 = s_1 - s_2 - s_3 = -F_0 + 2 F_1 - F_3
// -- three accumulator clears and half of the output-transform adds less per N-tile.  The bias (when this wavefront carries
// it: K-split layers add it once) enters component (1, 1)'s accumulator before pass 1: F_1, F_2, F_3 then carry it once in
// both columns.
// FENCE (the cost net's rounds): a scheduling fence between a pass and its fold.
template <int NN, int T0, int T1, unsigned KSTEP = WG_KSTEP, bool FENCE = false>
__device__ __forceinline__ void wg_round(unsigned (&RA)[3][4], __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned wp_after, unsigned lofs, int niter,
                                         int wstride, unsigned pstride, const float* __restrict__ bias_lane, wgf4 (&W)[NN][2], wgf4 (&Y)[NN][3][2][2])
{
    using std::integral_constant;
    wgf2 D[2][4];                                               // window rows A1 (columns 0-1, 2-3) and A2 of two steps in flight
    // the lane's four biases per N-tile: fetched per round and only alive through pass 0, when no partial output exists yet
    wgf4 bv[NN];
#pragma unroll
    for (int n = 0; n < NN; n++) bv[n] = bias_lane ? *reinterpret_cast<const wgf4*>(bias_lane + n * 16) : (wgf4){ 0.f, 0.f, 0.f, 0.f };
    wgf4 acc[NN][3][4];
    // (an opaque zero: folded into the first MFMA as the constant C = 0, the accumulators -- accumulation registers since the
    // paired layers park their outputs there -- become loop-carried copies: 36-68 v_accvgpr moves per iteration of every pass 0)
    float zero = 0.f;
    asm volatile("" : "+v"(zero));
#pragma unroll
    for (int n = 0; n < NN; n++)
#pragma unroll
        for (int t = T0; t < T1; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[n][t][j] = (wgf4){ zero, zero, zero, zero };
    auto run = [&](auto ic) __attribute__((always_inline)) {
        constexpr int I = decltype(ic)::value;
        constexpr int INEXT = I == 3 ? 0 : I + 1;
        if constexpr (I == 1) {
#pragma unroll
            for (int n = 0; n < NN; n++)
#pragma unroll
                for (int t = T0; t < T1; t++) acc[n][t][1] += bv[n];
        }
        constexpr int ICHAIN = (INEXT != 0 && wg_chains(I)) ? INEXT : -1;      // the next row component of this round, if any
        wg_pass<I, NN, T0, T1, wg_chains(I - 1), ICHAIN, KSTEP>(RA, rs, wp + I * pstride, INEXT == 0 ? wp_after : wp + (I + 1) * pstride, lofs, niter, wstride, W, acc, D);
        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);     // the fold is not mixed into the pass's end (the cost net spills without it)
#pragma unroll
        for (int n = 0; n < NN; n++)
#pragma unroll
            for (int t = T0; t < T1; t++) {
                const wgf4 f0 = acc[n][t][0] + acc[n][t][1] + acc[n][t][2];
                const wgf4 f1 = acc[n][t][1] - acc[n][t][2] - acc[n][t][3];
                if constexpr (I == 0) { Y[n][t][1][0] = f0; Y[n][t][1][1] = f1; }                 // F_0 (enters with a minus sign below)
                else if constexpr (I == 1) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        Y[n][t][1][0][r] = __builtin_fmaf(2.f, f0[r], -Y[n][t][1][0][r]);
                        Y[n][t][1][1][r] = __builtin_fmaf(2.f, f1[r], -Y[n][t][1][1][r]);
                    }
                }
                else if constexpr (I == 2) { Y[n][t][0][0] = f0; Y[n][t][0][1] = f1; }
                else { Y[n][t][1][0] -= f0; Y[n][t][1][1] -= f1; }
                // the folded values exist HERE and are pinned: left free, the compiler sinks these sums below the next pass's loop and
                // carries the accumulators of this pass (twice the registers) through it instead -- copies (+0.8 % on k_cyl_net_wg)
                // and, in the cost net, spills
                if constexpr (I == 2) asm volatile("" : "+v"(Y[n][t][0][0]), "+v"(Y[n][t][0][1]));
                else asm volatile("" : "+v"(Y[n][t][1][0]), "+v"(Y[n][t][1][1]));
            }
    };
    run(integral_constant<int, 0>{});
    run(integral_constant<int, 1>{});
    run(integral_constant<int, 2>{});
    run(integral_constant<int, 3>{});
}

// M-tile 2 is output row 6, columns 0..15 (columns 16..19 are the two Winograd tiles that ride in M-tile 1), in the DIRECT form: its
// window ends in the elevation padding (row 7), so two filter rows x three azimuth taps are all there is,
//     y[o][6][p] = b[o] + sum_c sum_{a = 0, 1} sum_{b = 0, 1, 2} g[o][c][a][b] * x[c][5 + a][p - 1 + b],          p = 0..15
// and the 16 positions fill the M-tile: 6 matrix instructions per (4 input, 16 output channels) where the eight Winograd tiles of
// these positions took 8 in half-empty ones.  Lane (li, lk) holds position p = li and channel lk of the k-step; a tap's operand is an
// LDS word as it stands (row * 22 + p + {0, 1, 2}: the halo word in front of column 0 serves p - 1 at p = 0) -- no input transform,
// no output fold.  The reads are 4-byte ones: nothing aligns p.  Within one read the 16 lanes of a channel are on consecutive banks;
// the two channels of a half-wave share them (ds_read_b32 banks by word mod 32 and the channel stride is 0 mod 32), a two-way
// conflict on 6 reads per k-step that the LDS has room for.
// The six taps are formed in registers from the Winograd blocks the filter set already has, U_ij = (G g G^T)_ij:
//     g[0][0] = U_00    g[0][1] = U_01 - U_02    g[0][2] = U_03        and with D_j = U_1j - U_2j
//     g[1][0] = D_0     g[1][1] = D_1 - D_2      g[1][2] = D_3
// (six subtractions per N-tile and k-step.  Nothing is stored for this round: a fifth block, U_1 - U_2, once made the filter set
// 3.8 MB -- more than the 4 MB L2 of an XCD holds beside the activation stream -- and the kernel's HBM-side traffic went from 47
// to 85 KB per patch.)
// One accumulator per filter row, K ascending, taps b = 0, 1, 2 in this order within a k-step -- the same for every N-tile and layer
// form; the bias starts in row 0's accumulator and the two are added once at the end.  (Two chains per N-tile: the dependent latency
// of v_mfma_f32_16x16x4_f32 is 40 cycles against 32 of issue, and a wavefront with one N-tile has nothing else to put between.)
// Steps are k-steps, pipelined as in wg_pass: the MFMAs of step s back to back, then the LDS reads of step s + 2 into the operand
// registers just consumed, then the taps of step s + 1, whose weight registers (a ring of two k-steps per block) are reloaded with
// the k-step two further on.  On entry W holds block 0's first two k-steps (the look-ahead of the round before).
typedef const __attribute__((address_space(3))) float* wg_lds_f1;
#define WG_LOADD(DST, A0, OFS)                                                                            \
    {                                                                                                     \
        _Pragma("unroll") for (int a_ = 0; a_ < 2; a_++)                                                  \
            _Pragma("unroll") for (int b_ = 0; b_ < 3; b_++)                                              \
                DST[a_ * 3 + b_] = *(wg_lds_f1)(size_t)((A0) + (OFS) + 4 * (a_ * WG_ROW + b_));           \
    }
template <int NN>
__device__ __forceinline__ void wg_round_direct(unsigned row5, __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned lofs, int niter, int wstride,
                                                unsigned pstride, const float* __restrict__ bias_lane, wgf4 (&W)[NN][2], wgf4 (&Y)[NN])
{
    wgf4 Wr[3][NN][2];                                          // blocks 0..2, two k-steps each
#pragma unroll
    for (int n = 0; n < NN; n++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            Wr[0][n][k] = W[n][k];
            Wr[1][n][k] = wg_ldw(rs, wp + pstride + n * 256 + k * wstride, lofs);
            Wr[2][n][k] = wg_ldw(rs, wp + 2 * pstride + n * 256 + k * wstride, lofs);
        }
    float X[2][6];                                              // window words [row 5 | row 6][tap] of two steps in flight
    unsigned pa = row5;
    WG_LOADD(X[0], pa, 0)
    WG_LOADD(X[1], pa, WG_KSTEP)
    wgf4 acc[NN][2];
    float zero = 0.f;
    asm volatile("" : "+v"(zero));
#pragma unroll
    for (int n = 0; n < NN; n++) {
        acc[n][0] = bias_lane ? *reinterpret_cast<const wgf4*>(bias_lane + n * 16) : (wgf4){ zero, zero, zero, zero };
        acc[n][1] = (wgf4){ zero, zero, zero, zero };
    }
    float G[NN][6];
#define WG_TAPS(SLOT)                                                                                     \
    _Pragma("unroll") for (int n = 0; n < NN; n++) {                                                      \
        const wgf4 u0_ = Wr[0][n][SLOT], u1_ = Wr[1][n][SLOT], u2_ = Wr[2][n][SLOT];                      \
        const float d1_ = wg_sub(u1_[1], u2_[1]), d2_ = wg_sub(u1_[2], u2_[2]);                           \
        G[n][0] = u0_[0]; G[n][1] = wg_sub(u0_[1], u0_[2]); G[n][2] = u0_[3];                             \
        G[n][3] = wg_sub(u1_[0], u2_[0]); G[n][4] = wg_sub(d1_, d2_); G[n][5] = wg_sub(u1_[3], u2_[3]);   \
    }
#define WG_RELOAD(SLOT, OFS)                                                                              \
    _Pragma("unroll") for (int n = 0; n < NN; n++)                                                        \
        _Pragma("unroll") for (int blk = 0; blk < 3; blk++) Wr[blk][n][SLOT] = wg_ldw(rs, (OFS) + blk * pstride + n * 256, lofs);
    WG_TAPS(0)
    WG_RELOAD(0, wp + 2 * wstride)
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
                    for (int n = 0; n < NN; n++)
                        acc[n][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(G[n][a * 3 + b], X[s & 1][a * 3 + b], acc[n][a], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (s < 2) WG_LOADD(X[s & 1], pa, (s + 2) * WG_KSTEP)
            else {
                if (s == 2) pa += adv;                           // the next iteration's base from here on
                WG_LOADD(X[s & 1], pa, (s - 2) * WG_KSTEP)
            }
            __builtin_amdgcn_sched_barrier(0);
            WG_TAPS((s + 1) & 1)                                 // k-step s + 1's taps; its registers take the k-step two further on
            if (s == 0) WG_RELOAD(1, wcur + 3 * wstride)
            else WG_RELOAD((s + 1) & 1, wn + (s - 1) * wstride)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef WG_TAPS
#undef WG_RELOAD
#pragma unroll
    for (int n = 0; n < NN; n++) Y[n] = acc[n][0] + acc[n][1];
}

// ReLU + store of one N-tile's outputs: into the activation buffer (with the circular halo copies) or to y[32][140].
// The weights are the MFMA's first operand, so the C/D layout has lane column li = the tile and rows lk * 4 + r = the
// output channel: a store instruction writes 16 different positions of a channel (distinct banks), not 16 channels at one
// position (one bank: the channel stride is a multiple of 32 words).
template <bool GLB>
__device__ __forceinline__ void wg_store_tile(const wgf4 (&Yt)[2][2], int t, int nt, int relu, float* __restrict__ act, float* __restrict__ out_glb,
                                              int li, int lk)
{
    const int n0 = nt * 16 + lk * 4;
    const float lo = relu ? 0.f : -__builtin_inff();
    {
        int ty, tx;
        const bool valid = wg_tile(t, li, ty, tx);
#pragma unroll
        for (int u = 0; u < 2; u++) {                             // (the tiles of tile row 3 in M-tile 1: their second output row is row 7)
            const int row = 2 * ty + u;
            const bool ok = valid && row < 7;
            if constexpr (GLB) {
                if (ok) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float v0 = fmaxf(Yt[u][0][r], lo), v1 = fmaxf(Yt[u][1][r], lo);
                        // (plain stores: the L2 combines these 8-byte pieces into lines; as non-temporal stores they left as partial
                        // writes, 38 instead of 17.5 KB of WRITE_SIZE per patch)
                        *reinterpret_cast<wgf2*>(out_glb + (size_t)(n0 + r) * 140 + row * 20 + 2 * tx) = (wgf2){ v0, v1 };
                    }
                }
            } else {
                // straight-line code (a branch per store costs more than the store): lanes with nothing to write, and the halo
                // copies of the inner tiles, go to the two dump words behind the channel's zero area
                const int pos = ok ? row * WG_ROW + 2 * tx + 1 : WG_ZERO + 4;
                const int h0 = (ok && tx == 0) ? row * WG_ROW + 21 : WG_ZERO + 4;      // column 0 again behind column 19
                const int h1 = (ok && tx == 9) ? row * WG_ROW : WG_ZERO + 5;           // column 19 again in front of column 0
                float* p = act + n0 * WG_CS;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float v0 = fmaxf(Yt[u][0][r], lo), v1 = fmaxf(Yt[u][1][r], lo);
                    p[r * WG_CS + pos] = v0; p[r * WG_CS + pos + 1] = v1;
                    p[r * WG_CS + h0] = v0; p[r * WG_CS + h1] = v1;
                }
            }
        }
    }
}

// The same for M-tile 2 (wg_round_direct): the C/D layout there has lane column li = output column li of row 6, one value per
// register.  Column 0 goes behind column 19 as well; column 19 and its copy in front of column 0 belong to M-tile 1.
template <bool GLB>
__device__ __forceinline__ void wg_store_row6(const wgf4& Yr, int nt, int relu, float* __restrict__ act, float* __restrict__ out_glb, int li, int lk)
{
    const int n0 = nt * 16 + lk * 4;
    const float lo = relu ? 0.f : -__builtin_inff();
    if constexpr (GLB) {
#pragma unroll
        for (int r = 0; r < 4; r++) out_glb[(size_t)(n0 + r) * 140 + 6 * 20 + li] = fmaxf(Yr[r], lo);
    } else {
        const int pos = 6 * WG_ROW + li + 1;
        const int h0 = li == 0 ? 6 * WG_ROW + 21 : WG_ZERO + 4;   // (lanes with no halo copy to make: the dump word)
        float* p = act + n0 * WG_CS;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float v = fmaxf(Yr[r], lo);
            p[r * WG_CS + pos] = v; p[r * WG_CS + h0] = v;
        }
    }
}

// All three M-tiles of one N-tile into the activation buffer
__device__ __forceinline__ void wg_store(const wgf4 (&Y)[3][2][2], int nt, int relu, float* __restrict__ act, int li, int lk)
{
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (t == 2) wg_store_row6<false>(Y[t][0][0], nt, relu, act, nullptr, li, lk);     // (the one quad of M-tile 2 rides in slot [0][0])
        else wg_store_tile<false>(Y[t], t, nt, relu, act, nullptr, li, lk);
    }
}

// The 9 window-row addresses depend on the lane only (the map's geometry is the same in every layer): formed ONCE per kernel and parked in
// accumulation registers (round 6); a layer reads them back (one v_accvgpr_read each, plus one add where its K range does not
// start at channel 0) instead of re-deriving tile coordinates and padding selects -- ~110 vector instructions per layer and wavefront.
struct WgAddrPark { float a[3][4]; };
__device__ __forceinline__ void wg_park_addresses(const float* act, int li, int lk, WgAddrPark& pk)
{
    const unsigned act_addr = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)act;
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int a = 0; a < (t == 2 ? 1 : 4); a++) {
            const unsigned v = wg_row_addr(act_addr, t, a, li, lk);
            asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(pk.a[t][a]) : "v"(v));
        }
}
__device__ __forceinline__ unsigned wg_parked(const WgAddrPark& pk, int t, int a)
{
    unsigned v;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(pk.a[t][a]));
    return v;
}

template <int NN, int K0, int K1, int KN>
__device__ __forceinline__ void wg_first_weights(__amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned lofs, int wstride, wgf4 (&W)[NN][KN])
{
#pragma unroll
    for (int n = 0; n < NN; n++)
#pragma unroll
        for (int k = K0; k < K1; k++) W[n][k] = wg_ldw(rs, wp + n * 256 + k * wstride, lofs);
}

// One layer with 32 output channels (two N-tiles, four wavefronts), the M-split pair form inside each half of K: wavefront (h, half)
// owns BOTH N-tiles for the Winograd M-tile h and the bottom row of N-tile h, over its half of K.  The upper half hands its partial
// sums (nine quads: 4 + 4 of the Winograd M-tile, one of row 6) to the lower one through the rows of the channels >= 64 (free:
// Cin <= 64), which adds them and stores; the bias rides in the lower half's accumulators.  (One N-tile per wavefront over all three
// M-tiles pays a transform per 4 MFMAs instead of 8.  Round 2 split the M-tiles {0} | {1, 2} over the wavefront pair instead: 16
// against 28 tile-components, the layer took 28 / 22 of its balanced time -- these two layers are 6.5 % of the MFMAs and were 11 %
// of the kernel.)
#define WG_XCH_C 64
template <bool GLB>
__device__ __forceinline__ void wg_layer_mksplit(float* __restrict__ act, float* __restrict__ out_glb, const float* __restrict__ wt,
                                                 const float* __restrict__ bias, int cin, int cout, int relu, int w, const WgAddrPark& pk)
{
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int li = lane & 15, lk = lane >> 4;
    const int h = w & 1, half = w >> 1;
    const int k4 = cin >> 2, kn = k4 >> 1, k0 = half * kn, wstride = 512;
    unsigned RA[3][4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const unsigned r0 = wg_parked(pk, 0, a), r1 = wg_parked(pk, 1, a);
        RA[0][a] = (h ? r1 : r0) + (unsigned)k0 * WG_KSTEP; RA[1][a] = RA[0][a];
    }
    RA[2][0] = wg_parked(pk, 2, 0) + (unsigned)k0 * WG_KSTEP;
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned wp = (unsigned)k0 * wstride;                            // [pair 0][i][k-step][n2][lane][j]
    const unsigned wpb = wp + (unsigned)h * 256;
    const unsigned lofs = lane * 16;
    const unsigned pstride = (unsigned)(k4 * wstride);
    wgf4 Y[2][3][2][2];
    wgf4 W2[2][2];
    wg_first_weights<2, 0, 2>(rs, wp, lofs, wstride, W2);
    wg_round<2, 0, 1>(RA, rs, wp, wpb, lofs, kn >> 2, wstride, pstride, half ? nullptr : bias + lk * 4, W2, Y);               // slot 0 = M-tile h
    wgf4 W1[1][2] = { { W2[0][0], W2[0][1] } };
    wgf4 Yb[1];
    wg_round_direct<1>(RA[2][0], rs, wpb, lofs, kn >> 2, wstride, pstride, half ? nullptr : bias + h * 16 + lk * 4, W1, Yb);
    wgf4* slot = reinterpret_cast<wgf4*>(act + WG_XCH_C * WG_CS) + h * 640 + lane;                   // 9 x 64 float4 per wavefront pair (in slots of 10)
    if (half) {
#pragma unroll
        for (int q = 0; q < 8; q++) slot[q * 64] = Y[q >> 2][0][(q >> 1) & 1][q & 1];
        slot[8 * 64] = Yb[0];
    }
    __syncthreads();                                 // partial sums are in place AND every wavefront has finished reading the input
    if (!half) {
#pragma unroll
        for (int q = 0; q < 8; q++) Y[q >> 2][0][(q >> 1) & 1][q & 1] += slot[q * 64];
        Yb[0] += slot[8 * 64];
        wg_store_tile<GLB>(Y[0][0], h, 0, relu, act, out_glb, li, lk);
        wg_store_tile<GLB>(Y[1][0], h, 1, relu, act, out_glb, li, lk);
        wg_store_row6<GLB>(Yb[0], h, relu, act, out_glb, li, lk);
    }
}

// One layer with 64 output channels (four N-tiles, four wavefronts): wavefront w owns the N-tile pair w & 1 for ONE of the
// M-tiles 0, 1 (w >> 1) -- the transform of a step feeds 8 MFMAs, as in the 128-channel layers -- and row 6 (M-tile 2, the direct form) of
// ONE N-tile of its pair: 32 + 6 = 38 matrix instructions per k-step for every wavefront, no partial sums to exchange.
// (One N-tile per wavefront over all M-tiles, the round-2 form, pays 1.8 transform instructions per MFMA instead of 1.0.)
__device__ __forceinline__ void wg_layer_msplit(float* __restrict__ act, const float* __restrict__ wt, const float* __restrict__ bias,
                                                int cin, int cout, int relu, int w, const WgAddrPark& pk)
{
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int li = lane & 15, lk = lane >> 4;
    const int pair = w & 1, h = w >> 1;
    const int k4 = cin >> 2, wstride = 512;
    unsigned RA[3][4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const unsigned r0 = wg_parked(pk, 0, a), r1 = wg_parked(pk, 1, a);
        RA[0][a] = h ? r1 : r0; RA[1][a] = RA[0][a];
    }
    RA[2][0] = wg_parked(pk, 2, 0);
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned wp = (unsigned)pair * (WG_BLOCKS * cin * 32);           // [pair][i][k-step][n2][lane][j]
    const unsigned wpb = wp + (unsigned)h * 256;                           // the N-tile of the pair whose bottom row is this wavefront's
    const unsigned lofs = lane * 16;
    const unsigned pstride = (unsigned)(k4 * wstride);
    wgf4 Y[2][3][2][2];
    wgf4 W2[2][2];
    wg_first_weights<2, 0, 2>(rs, wp, lofs, wstride, W2);
    wg_round<2, 0, 1>(RA, rs, wp, wpb, lofs, k4 >> 2, wstride, pstride, bias + (2 * pair) * 16 + lk * 4, W2, Y);     // slot 0 = M-tile h
    wgf4 W1[1][2] = { { W2[0][0], W2[0][1] } };
    wgf4 Yb[1];
    wg_round_direct<1>(RA[2][0], rs, wpb, lofs, k4 >> 2, wstride, pstride, bias + (2 * pair + h) * 16 + lk * 4, W1, Yb);
    __syncthreads();                                 // every wavefront has finished reading the layer's input
    wg_store_tile<false>(Y[0][0], h, 2 * pair, relu, act, nullptr, li, lk);
    wg_store_tile<false>(Y[1][0], h, 2 * pair + 1, relu, act, nullptr, li, lk);
    wg_store_row6<false>(Yb[0], 2 * pair + h, relu, act, nullptr, li, lk);
}

// N-tiles per wavefront of a layer: every layer form owns N-tile pairs.  The filter tiling follows it (buf_winograd_tile_weights).
// (For the 64-channel layers, pairs with K split over two wavefronts and the partial sums exchanged through the dead half of the
// buffer measured 1 % slower than the M split, before and after the filter stream became cheap: short K loops, a third barrier.)
__host__ __device__ constexpr int wg_group(int cin, int cout) { return 2; }

// Outputs of M-tile T of both N-tiles of a pair -> accumulation registers (see wg_layer_pair)
template <int T>
__device__ __forceinline__ void wg_park(const wgf4 (&Y)[2][3][2][2], float (&park)[2][3][16])
{
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int q = 0; q < (T == 2 ? 4 : 16); q++)             // (M-tile 2: the one quad of row 6)
            asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][T][q]) : "v"(Y[n][T][q >> 3][(q >> 2) & 1][q & 3]));
}

// One layer with 128 output channels: wavefront w owns the N-tile pair 2w, 2w+1 over the whole K, and the transform of a step
// feeds 8 MFMAs.  The held outputs (72 registers) wait in accumulation registers; the two Winograd M-tiles share one round
// (64 accumulators; a round per M-tile -- more passes, the pair's filters streamed a third time -- measured 0.9 % slower), row 6
// (M-tile 2, the direct form) is the second.
__device__ __forceinline__ void wg_layer_pair(float* __restrict__ act, const float* __restrict__ wt, const float* __restrict__ bias,
                                              int cin, int cout, int relu, int pair, const WgAddrPark& pk)
{
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int k4 = cin >> 2, wstride = 512;
    unsigned RA[3][4];
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int a = 0; a < (t == 2 ? 1 : 4); a++) RA[t][a] = wg_parked(pk, t, a);
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned wp = (unsigned)pair * (WG_BLOCKS * cin * 32);           // [pair][i][k-step][n2][lane][j]
    const unsigned lofs = lane * 16;
    const unsigned pstride = (unsigned)(k4 * wstride);
    wgf4 Y[2][3][2][2];
    const float* bv = bias + (2 * pair) * 16 + lk * 4;
    wgf4 W1[2][2];
    wg_first_weights<2, 0, 2>(rs, wp, lofs, wstride, W1);
    // The outputs of a finished round wait for the in-place barrier in ACCUMULATION registers (v_accvgpr_write / _read: the unified
    // file gives a wavefront 256 registers of either kind): left in VGPRs the compiler parked 19 of the then 20 quads in scratch memory
    // (264 KB of HBM traffic per patch); the rounds then run in ~130 VGPRs with no scratch at all.
    float park[2][3][16];
    wg_round<2, 0, 2>(RA, rs, wp, wp, lofs, k4 >> 2, wstride, pstride, bv, W1, Y);     // both Winograd M-tiles in one round
    wg_park<0>(Y, park);
    wg_park<1>(Y, park);
    wgf4 Yb[2];
    wg_round_direct<2>(RA[2][0], rs, wp, lofs, k4 >> 2, wstride, pstride, bv, W1, Yb);
    Y[0][2][0][0] = Yb[0]; Y[1][2][0][0] = Yb[1];
    wg_park<2>(Y, park);
    __syncthreads();                                 // every wavefront has finished reading the layer's input
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the store offsets are formed here, not kept (spilled) from the layer's start
#pragma unroll
    for (int n = 0; n < 2; n++) {
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int q = 0; q < (t == 2 ? 4 : 16); q++)
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(Y[n][t][q >> 3][(q >> 2) & 1][q & 3]) : "a"(park[n][t][q]));
        wg_store(Y[n], 2 * pair + n, relu, act, lane_s & 15, lane_s >> 4);
    }
}

// The patch's input into the activation buffer, the zero words of every channel, and the barrier behind them
__device__ __forceinline__ void wg_load_input(const float* __restrict__ x, const CylWgParams& P, float* __restrict__ act, int patch)
{
    {   // input [48][140] -> rows of 22 with the halo columns.  A row is five float4: every load of the patch is issued before the
        // first LDS store (one load at a time, each behind the previous one's stores, took 40 k cycles per patch: 5 % of the kernel)
        const wgf4* src = reinterpret_cast<const wgf4*>(x + (size_t)patch * P.cin[0] * 140);
        const int nq = P.cin[0] * 35;                               // float4 per patch (7 per thread for the 48 channels of this network)
        wgf4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = threadIdx.x + k * WG_THREADS;
            if (i < nq) v[k] = __builtin_nontemporal_load(src + i);    // streamed once: leave the L2 to the filters
        }
        auto put = [&](int i, wgf4 u) __attribute__((always_inline)) {
            const int c = i / 35, q = i - c * 35;
            const int row = q / 5, col = (q - row * 5) * 4;
            float* p = act + c * WG_CS + row * WG_ROW + col + 1;
            p[0] = u[0]; p[1] = u[1]; p[2] = u[2]; p[3] = u[3];
            if (col == 0) p[20] = u[0];
            if (col == 16) p[-17] = u[3];
        };
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = threadIdx.x + k * WG_THREADS;
            if (i < nq) put(i, v[k]);
        }
        for (int i = threadIdx.x + 8 * WG_THREADS; i < nq; i += WG_THREADS) put(i, __builtin_nontemporal_load(src + i));   // wider first layers
    }
    for (int i = threadIdx.x; i < WG_MAXC * 4; i += WG_THREADS) act[(i >> 2) * WG_CS + WG_ZERO + (i & 3)] = 0.f;
    __syncthreads();
}

__device__ __forceinline__ void cyl_net_wg_body(const float* __restrict__ x, const CylWgParams& P, float* __restrict__ y, float* __restrict__ lds)
{
    float* act = lds;                                // [128][160]
    const int patch = blockIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    WG_STAMP_AT(17)
#ifdef WG_STAMP
    if (threadIdx.x == 0) { P.stamps[(size_t)gridDim.x * 80 + blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memtime(); P.stamps[(size_t)gridDim.x * 80 + blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime(); }
#endif
    wg_load_input(x, P, act, patch);
    WG_STAMP_AT(0)
    WgAddrPark pk;
    {
        int lane0 = threadIdx.x & (WAVE - 1);
        asm volatile("" : "+v"(lane0));
        wg_park_addresses(act, lane0 & 15, lane0 >> 4, pk);
    }
#pragma unroll 1
    for (int l = 0; l < WG_LAYERS; l++) {
        const int cin = P.cin[l], cout = P.cout[l];
        if (cout == 128) wg_layer_pair(act, P.wt[l], P.bias[l], cin, cout, P.relu[l], w, pk);
        else if (cout == 64) wg_layer_msplit(act, P.wt[l], P.bias[l], cin, cout, P.relu[l], w, pk);
        else if (l < WG_LAYERS - 1) wg_layer_mksplit<false>(act, nullptr, P.wt[l], P.bias[l], cin, cout, P.relu[l], w, pk);
        else wg_layer_mksplit<true>(act, y + (size_t)patch * cout * 140, P.wt[l], P.bias[l], cin, cout, P.relu[l], w, pk);
        WG_STAMP_AT(2 * l + 1)
        __syncthreads();
        WG_STAMP_AT(2 * l + 2)
    }
#ifdef WG_STAMP
    if (threadIdx.x == 0) { P.stamps[(size_t)gridDim.x * 80 + blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memtime(); P.stamps[(size_t)gridDim.x * 80 + blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime(); }
#endif
}

__global__ void __launch_bounds__(WG_THREADS, 2) k_cyl_net_wg(const float* __restrict__ x, CylWgParams P, float* __restrict__ y)
{
    extern __shared__ float lds[];
    cyl_net_wg_body(x, P, y, lds);
}

// The masked re-run of buf_cylindrical_net_split_safe: the same body for the patches the split-f16 kernel flagged (P.only_if[patch] != 0),
// nothing else.  Its own kernel NAME: the launch covers the full grid and is empty in the normal case -- under the name of k_cyl_net_wg
// it would be averaged into that kernel's time, traffic and instruction counts in every profile.
__global__ void __launch_bounds__(WG_THREADS, 2) k_cyl_net_wg_rerun(const float* __restrict__ x, CylWgParams P, float* __restrict__ y)
{
    extern __shared__ float lds[];
    if (P.only_if[blockIdx.x] == 0) return;
    cyl_net_wg_body(x, P, y, lds);
}


// Host helper: filters w [Cout][Cin][3][3] (BN folded) -> U = G g G^T in fp64, rounded once, in the kernel's A-operand tiling
//     out[16 * Cout * Cin] = [N-group][i][k-step][n2][lk][li][j] = U[i][j][16 (NG g + n2) + li][4 ks + lk]
// with N-groups of NG = 2 N-tiles for 128 output channels (a wavefront owns a pair there) and NG = 1 otherwise: the
// k-steps of a wavefront follow each other in memory (round 2 had the N-tile inside the k-step: every 1 KB fetch of a
// wavefront then sat on another 4-8 KB page, and the filter stream cost 8 % of the kernel in translation misses).  No device work.
// General form: N-groups of ng N-tiles; nblk = 4, or 5 with g[1] G^T (= U_1 - U_2, the filter row a window that ends in the
// padding sees: the kernels form it in registers) as block 4; out[4 nblk * Cout * Cin].
extern "C" int buf_winograd_tile_filters(const float* w_host, int cout, int cin, int ng, int nblk, float* out_host)
{
    BUF_REQUIRE(w_host && out_host, BUF_EINVAL, "buf_winograd_tile_filters: null argument");
    BUF_REQUIRE(cout > 0 && cin > 0 && cout % 16 == 0 && cin % 4 == 0, BUF_EINVAL, "buf_winograd_tile_filters: widths %d -> %d", cin, cout);
    BUF_REQUIRE(ng >= 1 && (cout / 16) % ng == 0 && (nblk == 4 || nblk == 5), BUF_EINVAL, "buf_winograd_tile_filters: %d N-tiles in groups of %d, %d blocks",
                cout / 16, ng, nblk);
    static const double G[4][3] = { { 1, 0, 0 }, { .5, .5, .5 }, { .5, -.5, .5 }, { 0, 0, 1 } };
    const int k4 = cin / 4;
    for (int o = 0; o < cout; o++)
        for (int c = 0; c < cin; c++) {
            const float* g = w_host + ((size_t)o * cin + c) * 9;
            const int n = o / 16;
            for (int i = 0; i < nblk; i++)
                for (int j = 0; j < 4; j++) {
                    double u = 0;
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) u += (i < 4 ? G[i][a] : (a == 1 ? 1.0 : 0.0)) * (double)g[3 * a + b] * G[j][b];
                    const size_t idx = ((((((size_t)(n / ng) * nblk + i) * k4 + c / 4) * ng + n % ng) * 4 + c % 4) * 16 + o % 16);
                    out_host[idx * 4 + j] = (float)u;
                }
        }
    return BUF_OK;
}

extern "C" int buf_winograd_tile_weights(const float* w_host, int cout, int cin, float* out_host)
{
    BUF_REQUIRE(cout > 0 && cin > 0 && cout % 16 == 0 && cin % 4 == 0, BUF_EINVAL, "buf_winograd_tile_weights: widths %d -> %d", cin, cout);
    return buf_winograd_tile_filters(w_host, cout, cin, wg_group(cin, cout), WG_BLOCKS / 4, out_host);
}

// N-tiles per group in the filter tiling of a layer with these widths (the Python side asks instead of restating the rule)
extern "C" int buf_winograd_group(int cin, int cout) { return wg_group(cin, cout); }
