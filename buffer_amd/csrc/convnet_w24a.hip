// A11 dense part -- w24a_layer_psplit32, a layer form of the fused kernel (cyl_net_w25t_body, csrc/convnet_w25t.hip): F(2x4, 3x3) tiles in
// EVERY layer the caller hands an F(2x4) filter set for -- layer 0 and the 32-output layers of the released stack, which a stack without
// sets of its own runs in the F(2x2) form at 38 matrix instructions per (k-step, N-tile).  With all eight layers at 24 + 6 the released
// stack issues 30 x 736 = 22 080 matrix instructions per patch (without the sets: 22 848).
//
// The F(2x4) layer forms, picked per layer from the widths and the kernel's relu word (bit 2 there means "P.wt[l] IS the layer's F(2x4) set";
// the launcher sets it for the layers that carry BUF_CYL_F24K and for those with a set of their own, see cyl_prepare, csrc/cnn_launch.hip):
//   128 outputs                 w24_layer_pair (csrc/convnet_w24.hip), unchanged
//   64 outputs, bit 2           w24p_layer_psplit (csrc/convnet_w24p.hip), unchanged: its k-loop runs Cin / 16 times, so Cin = 48 (layer 0:
//                               three iterations), 32 and 16 (one iteration) go through it as 64 and 128 do
//   32 outputs, bit 2           w24a_layer_psplit32, below
//   anything else               wg_layer_msplit / wg_layer_mksplit (csrc/convnet_wg.hip), as in every other kernel
//
// w24a_layer_psplit32: the pass split over ONE N-tile pair.  Wavefront w owns row component I = w of the F(2,3) row transform for both
// N-tiles over the whole K: per k-step two window rows, one transform of 18 instructions, 6 x 2 = 12 MFMAs into 48 accumulators
// (vector registers: beside them the filter ring takes 24 and the window words and operands 24; the compiler places the matrix
// instructions and their wait states itself).  A4^T is folded once after the loop (f_I: 2 N-tiles x 4 columns x wgf4); the bias rides in
// column component 1 of row component 1.  Wavefront q = 0, 1 finishes N-tile q:  row 0 = (f_0 + f_1) + f_2,  row 1 = (f_1 - f_2) - f_3.
// The direct round (row 6, columns 0..15) is shared so that every wavefront issues the same number of MFMAs: wavefront w runs N-tile
// w & 1 over the K half w >> 1 (Cin % 32 == 0: the widths rule of 32-output layers), 6 MFMAs on half of the k-steps; the bias starts in
// the lower half, and the upper half hands its quad to the finisher.  Per wavefront and k-step 12 + 3, per (k-step, N-tile) 30.
//
// The exchange area: the rows of the channels 64..127, words 0..143 of each -- free for the whole layer, since Cin <= 64 and Cout = 32.
// Wavefront w writes the 16 rows from channel 64 + 16 w on; lane (row = lane >> 2, quarter = lane & 3) has 36 words from word
// 36 quarter on: [f_w of N-tile 0: 16][f_w of N-tile 1: 16][row 6 of the upper K half: 4].  A finisher does not write what it keeps.
// Words WG_ZERO..WG_ZERO + 3 and the two dump words of these channels are not touched, so -- unlike behind wg_layer_mksplit, whose
// exchange runs over the zero words of the channels 64..95 -- a wider layer may follow, as long as no 32-output layer of the older form
// has run earlier in the stack (cyl_check, csrc/cnn_launch.hip).
//
// Barriers per layer, beside the one that closes every layer:
//   1. behind the dump-word clear (the window rows in the elevation padding read six words from the zero area on: w24_layer_pair);
//   2. behind the exchange writes: the partial outputs are in place AND every wavefront has finished reading the layer's input.
// No store can reach a word another wavefront still reads: the exchange writes go to rows no wavefront reads as input (Cin <= 64) and
// that the previous layer's finishers stopped reading before its closing barrier; each wavefront writes its own 16 rows only.  The
// finishers' stores (output rows 0..31 and their dump words, or global memory in the last layer) come behind barrier 2, when nobody reads
// the input any more, and the exchange rows they read are not written again before the closing barrier.
#include "common.h"

#define W24A_XCH_C 64          // first channel row of the exchange area
#define W24A_XCH_WORDS 36      // words per lane there (nine float4)

// w24p_pass for ONE N-tile pair: row component da + sgn db over `niter` x 4 k-steps, acc[n][j] += V_Ij(tile, c) * U_Ij(c, n).  The same
// steps, fences and transform (W24P_XFORM; the LDS reads one k-step ahead, the filter ring two); the accumulators are the compiler's.
// On entry W holds the first two k-steps of the block at wp; the last iteration fetches the k-steps 0, 1 at wp_next into the ring
// instead (unused, in bounds).
__device__ __forceinline__ void w24a_pass(unsigned P0, unsigned P1, float sgn, __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned wp_next, unsigned lofs4,
                                          unsigned lofs2, int niter, wgf4 (&W4)[2][2], wgf2 (&W2)[2][2], wgf4 (&acc)[2][6])
{
    wgf2 D[6];
    float V[2][6];
    W24_LOAD(D, P0, P1, 0)
    W24P_XFORM(0)
    int it = 0;
#pragma unroll 1
    do {                                             // (niter >= 1, as in w24p_pass)
        const bool more = it + 1 < niter;
        const unsigned wcur = wp + 4 * it * W24_WSTRIDE;                       // this iteration's k-steps 2, 3 ...
        const unsigned wn = more ? wcur + 4 * W24_WSTRIDE : wp_next;           // ... and the k-steps 0, 1 of the next one
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
            for (int n = 0; n < 2; n++)
#pragma unroll
                for (int j = 0; j < 6; j++)
                    acc[n][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(W24_U(n, s & 1, j), V[s & 1][j], acc[n][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            W24P_XFORM((s + 1) & 1)
#pragma unroll
            for (int n = 0; n < 2; n++) {                          // k-step s is through: its registers take the k-step two further on
                const unsigned o = s < 2 ? wcur + (s + 2) * W24_WSTRIDE : wn + (s - 2) * W24_WSTRIDE;
                W4[n][s & 1] = wg_ldw(rs, o + n * 256, lofs4);
                W2[n][s & 1] = w24_ldw2(rs, o + 512 + n * 128, lofs2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } while (++it < niter);
}

// ReLU + store of one finished N-tile: into the activation buffer (w24_store_tile, wg_store_row6) or, for the last layer, to y[32][140]
// -- a tile row is four floats at a 16-byte boundary there (140 nt + 20 row + 4 tx floats).
template <bool GLB>
__device__ __forceinline__ void w24a_store(const wgf4 (&Yk)[2][4], const wgf4& Yb, int nt, int relu, float* __restrict__ act, float* __restrict__ out_glb,
                                           int li, int lk)
{
    if constexpr (GLB) {
        const int n0 = nt * 16 + lk * 4;
        const float lo = relu ? 0.f : -__builtin_inff();
        int ty, tx;
        w24_tile(li, ty, tx);
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int row = 2 * ty + u;
            if (row < 7) {                           // (lane 15's second row is row 7)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    *reinterpret_cast<wgf4*>(out_glb + (size_t)(n0 + r) * 140 + row * 20 + 4 * tx) =
                        (wgf4){ fmaxf(Yk[u][0][r], lo), fmaxf(Yk[u][1][r], lo), fmaxf(Yk[u][2][r], lo), fmaxf(Yk[u][3][r], lo) };
            }
        }
    } else
        w24_store_tile(Yk, nt, relu, act, li, lk);
    wg_store_row6<GLB>(Yb, nt, relu, act, out_glb, li, lk);
}

// Wavefront Q = 0, 1 finishes N-tile Q: its own f_Q, the three received ones and the upper K half's quad of row 6
template <int Q, bool GLB>
__device__ __forceinline__ void w24a_take(const wgf4 (&f)[2][4], wgf4 Yb, int relu, float* __restrict__ act, float* __restrict__ out_glb, int lane)
{
    const float* xch = act + (W24A_XCH_C + (lane >> 2)) * WG_CS + (lane & 3) * W24A_XCH_WORDS;
    wgf4 Yk[2][4];
#pragma unroll
    for (int v = 0; v < 4; v++) {
        wgf4 F[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            F[i] = i == Q ? f[Q][v] : *reinterpret_cast<const wgf4*>(xch + 16 * i * WG_CS + 16 * Q + 4 * v);
        Yk[0][v] = (F[0] + F[1]) + F[2];
        Yk[1][v] = (F[1] - F[2]) - F[3];
    }
    Yb += *reinterpret_cast<const wgf4*>(xch + 16 * (Q + 2) * WG_CS + 32);
    w24a_store<GLB>(Yk, Yb, Q, relu, act, out_glb, lane & 15, lane >> 4);
}

// One layer with 32 output channels in the pass-split form; wt: the layer's F(2x4) set ([pair 0][i][k-step][768]).  Cin = 32 or 64.
template <bool GLB>
__device__ __forceinline__ void w24a_layer_psplit32(float* __restrict__ act, float* __restrict__ out_glb, const float* __restrict__ wt,
                                                    const float* __restrict__ bias, int cin, int relu, int w, const WgAddrPark& pk, const W24AddrPark& pk24)
{
    // (the dump words of the input channels: see w24_layer_pair)
    act[(threadIdx.x >> 1) * WG_CS + WG_ZERO + 4 + (threadIdx.x & 1)] = 0.f;
    __syncthreads();
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int k4 = cin >> 2, kn = k4 >> 1;
    const int nd = w & 1, half = w >> 1;             // the direct round's N-tile and K half
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned pstride = (unsigned)(k4 * W24_WSTRIDE);
    const unsigned wp = (unsigned)w * pstride;                                               // block (pair 0, i = w)
    const unsigned wpd = (unsigned)(half * kn) * W24_WSTRIDE + (unsigned)nd * 256;           // block 0 from the K half's first k-step on, N-tile nd's 16-byte part
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    // The direct round first, as in w24p_layer_psplit: its one quad waits through the pass
    const wgf4 W0[2] = { wg_ldw(rs, wpd, lofs4), wg_ldw(rs, wpd + W24_WSTRIDE, lofs4) };
    wgf4 Yb;
    w24p_round_direct<true>(wg_parked(pk, 2, 0) + (unsigned)(half * kn) * WG_KSTEP, rs, wpd, lofs4, kn >> 2, pstride,
                            half ? nullptr : bias + nd * 16 + lk * 4, W0, Yb);
    unsigned RA[4];
#pragma unroll
    for (int a = 0; a < 4; a++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(RA[a]) : "a"(pk24.a[a]));
    // window rows (da, db) of row component w: (0, 2) (1, 2) (2, 1) (1, 3); db enters with sgn
    const unsigned P0 = w == 0 ? RA[0] : (w == 2 ? RA[2] : RA[1]);
    const unsigned P1 = w == 3 ? RA[3] : (w == 2 ? RA[1] : RA[2]);
    const float sgn = w == 1 ? 1.f : -1.f;
    wgf4 f[2][4];                                    // f_w: [N-tile][column] after A4^T
    {
        wgf4 acc[2][6];
        float zero = 0.f;
        asm volatile("" : "+v"(zero));               // (an opaque zero: see wg_round)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int j = 0; j < 6; j++) acc[n][j] = (wgf4){ zero, zero, zero, zero };
        if (w == 1) {                                // the bias: once, in column component 1 of row component 1
#pragma unroll
            for (int n = 0; n < 2; n++) acc[n][1] = *reinterpret_cast<const wgf4*>(bias + n * 16 + lk * 4);
        }
        wgf4 W4[2][2];
        wgf2 W2[2][2];
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                W4[n][k] = wg_ldw(rs, wp + k * W24_WSTRIDE + n * 256, lofs4);
                W2[n][k] = w24_ldw2(rs, wp + k * W24_WSTRIDE + 512 + n * 128, lofs2);
            }
        w24a_pass(P0, P1, sgn, rs, wp, wp, lofs4, lofs2, k4 >> 2, W4, W2, acc);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 2; n++)
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
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the exchange and store offsets are formed here, not kept from the layer's start
    float* mine = act + (W24A_XCH_C + 16 * w + (lane_s >> 2)) * WG_CS + (lane_s & 3) * W24A_XCH_WORDS;
    if (w != 0) {
#pragma unroll
        for (int v = 0; v < 4; v++) *reinterpret_cast<wgf4*>(mine + 4 * v) = f[0][v];
    }
    if (w != 1) {
#pragma unroll
        for (int v = 0; v < 4; v++) *reinterpret_cast<wgf4*>(mine + 16 + 4 * v) = f[1][v];
    }
    if (half) *reinterpret_cast<wgf4*>(mine + 32) = Yb;
    __syncthreads();                                 // the partial outputs are in place AND every wavefront has finished reading the input
    if (w == 0) w24a_take<0, GLB>(f, Yb, relu, act, out_glb, lane_s);
    else if (w == 1) w24a_take<1, GLB>(f, Yb, relu, act, out_glb, lane_s);
}
