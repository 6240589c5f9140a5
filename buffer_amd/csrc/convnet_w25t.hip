// A11 dense part -- k_cyl_net_w25t, the fused kernel of every layer form (cyl_net_w25t_body below lists them), and the forms this file
// adds: two changes in the layers of 128 output channels (w24_layer_pair, csrc/convnet_w24.hip), each behind a bit of the kernel's relu
// word that only the launcher sets:
//
//   W25T_TAPS    the direct round of output row 6, columns 0..15 runs on taps the HOST formed.  Row 6's window is the map rows 5, 6 and
//                a padding row, so its six taps are rows 0 and 1 of the 3 x 3 filter as they stand,
//                    y[6][p] = b + sum_c sum_{a = 0, 1} sum_b w[a][b] x[c][5 + a][p - 1 + b]
//                w24_round_direct rebuilds them per patch, k-step and N-tile from three Winograd block rows (12 subtractions, six
//                16-byte loads and a ring of 48 registers per k-step and wavefront, three accumulators per N-tile closed by
//                4 acc_0 - 3 acc_1 + acc_2).  Here a lane loads its 12 taps of a k-step (two N-tiles) as three 16-byte words of a set of
//                its own (buf_cyl_row6_tile_taps, P.taps[l]): no tap arithmetic, a ring of 24 registers, and the taps are the filter's
//                own fp32 values, not differences of rounded blocks.
//   W25T_FIRST   the direct round runs IN FRONT of the Winograd round, as in the pass-split forms: its 8 outputs per lane wait in
//                accumulation registers, and the Winograd round's 64 go from its last fold straight to the barrier and the stores
//                (w24_layer_pair parks and fetches all 72: 128 more copies between the register files per wavefront and layer).
//
// A layer whose word carries neither bit runs w24_layer_pair itself: without a tap set and without the order bit the kernel returns
// the bits of the stack without them.
//
// Accumulators of the new direct round: one per AZIMUTH tap and N-tile, as in w24_round_direct (the filter rows a = 0, 1 add up in it, K
// ascending), summed once at the end, (acc_0 + acc_1) + acc_2; the bias starts acc_2.  One per N-tile would put the six matrix
// instructions of an N-tile in one dependent chain, two instructions apart in the issue order below; with three the distance stays the
// six of w24_round_direct, whose issue order and fences this round keeps.  (Not measured against each other.)
#include "common.h"

#define W25T_TAPS 16           // bit 4 of the kernel's relu word (set by the launcher only): P.taps[l] is the layer's row-6 tap set
#define W25T_FIRST 32          // bit 5: the direct round in front of the Winograd round
#define W25T_STRIDE 768        // floats per (N-tile pair, k-step) of a tap set: three 16-byte words per lane

// tap (a, b) of N-tile n in ring slot k: float n * 6 + a * 3 + b of the lane's twelve
#define W25T_G(n, k, a, b) T[k][((n) * 6 + (a) * 3 + (b)) >> 2][((n) * 6 + (a) * 3 + (b)) & 3]

// Output row 6, columns 0..15 of the N-tile pair in the direct form on host taps: w24_round_direct's window reads, steps and fences.
// Step s runs the 12 MFMAs of k-step s, reads the window words of k-step s + 2 into the operand registers just consumed and reloads
// the taps' ring slot with the k-step two further on.  rt / tp: the tap set and the pair's first k-step in it.
// The last iteration stands behind the loop (niter >= 2: Cin % 32 == 0): it fetches nothing past the round's end, and with PRIME its
// steps 2 and 3 fetch the first two k-steps of the Winograd round's block row 0 (rs, wp) into W4 / W2 instead.  (As a
// wavefront-uniform branch inside the loop the 24 registers of W4 / W2 were carried round it through the accumulation registers.)
template <bool PRIME>
__device__ __forceinline__ void w25t_round_direct(unsigned row5, __amdgpu_buffer_rsrc_t rt, unsigned tp, unsigned lofs4, int niter,
                                                  const float* __restrict__ bias_lane, wgf4 (&Y)[2], __amdgpu_buffer_rsrc_t rs, unsigned wp,
                                                  unsigned lofs2, wgf4 (&W4)[2][2], wgf2 (&W2)[2][2])
{
    wgf4 T[2][3];                                               // two k-steps of taps: [n2][a][b] as three 16-byte words
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int q = 0; q < 3; q++) T[k][q] = wg_ldw(rt, tp + k * W25T_STRIDE + q * 256, lofs4);
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
        acc[n][2] = *reinterpret_cast<const wgf4*>(bias_lane + n * 16);
    }
    // One iteration of four k-steps from the k-step at tcur on.  LAST: nothing of this round is fetched past its end.
    auto iteration = [&](auto last, unsigned tcur) __attribute__((always_inline)) {
        constexpr bool LAST = decltype(last)::value;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++) {
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int n = 0; n < 2; n++)
                        acc[n][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(W25T_G(n, s & 1, a, b), X[s & 1][a * 3 + b], acc[n][b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (s < 2) WG_LOADD(X[s & 1], pa, (s + 2) * WG_KSTEP)
            else if constexpr (!LAST) {
                if (s == 2) {                                    // the next iteration's base from here on; pinned: left free the loop's
                    pa += 4u * WG_KSTEP;                         // induction variable is rebased and every read gets an address add
                    asm volatile("" : "+v"(pa));
                }
                WG_LOADD(X[s & 1], pa, (s - 2) * WG_KSTEP)
            }
            __builtin_amdgcn_sched_barrier(0);
            // k-step s is through: its ring slot takes the k-step two further on
            if (s < 2 || !LAST) {
#pragma unroll
                for (int q = 0; q < 3; q++) T[s & 1][q] = wg_ldw(rt, tcur + (s + 2) * W25T_STRIDE + q * 256, lofs4);
            } else if constexpr (PRIME) {                        // the Winograd round's first steps instead (s & 1 = s - 2 here)
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    W4[n][s & 1] = wg_ldw(rs, wp + (s & 1) * W24_WSTRIDE + n * 256, lofs4);
                    W2[n][s & 1] = w24_ldw2(rs, wp + (s & 1) * W24_WSTRIDE + 512 + n * 128, lofs2);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
#pragma unroll 1
    for (int it = 0; it < niter - 1; it++) iteration(std::false_type{}, tp + 4 * it * W25T_STRIDE);
    iteration(std::true_type{}, tp + 4 * (niter - 1) * W25T_STRIDE);
#pragma unroll
    for (int n = 0; n < 2; n++) Y[n] = (acc[n][0] + acc[n][1]) + acc[n][2];
}

// w24_layer_pair with the direct round on host taps (TAPS: `taps` is the layer's set) and / or in front of the Winograd round (FIRST)
template <bool TAPS, bool FIRST>
__device__ __forceinline__ void w25t_layer_pair(float* __restrict__ act, const float* __restrict__ wt, const float* __restrict__ taps,
                                                const float* __restrict__ bias, int cin, int relu, int pair, const WgAddrPark& pk,
                                                const W24AddrPark& pk24)
{
    static_assert(TAPS || FIRST, "neither: w24_layer_pair");
    // (the dump words of the input channels and their barrier: see w24_layer_pair)
    act[(threadIdx.x >> 1) * WG_CS + WG_ZERO + 4 + (threadIdx.x & 1)] = 0.f;
    __syncthreads();
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int k4 = cin >> 2;
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const __amdgpu_buffer_rsrc_t rt = wg_weights(TAPS ? taps : wt);
    const unsigned pstride = (unsigned)(k4 * W24_WSTRIDE);
    const unsigned wp = (unsigned)pair * 4 * pstride;                      // [pair][i][k-step][...]
    const unsigned tp = (unsigned)(pair * k4) * W25T_STRIDE;               // [pair][k-step][...]
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    const float* bv = bias + (2 * pair) * 16 + lk * 4;
    wgf4 W4[2][2];
    wgf2 W2[2][2];
    wgf4 Y[2][2][4];
    wgf4 Yb[2];
    float park[2][36];
    auto first_steps = [&](bool narrow) __attribute__((always_inline)) {
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                W4[n][k] = wg_ldw(rs, wp + k * W24_WSTRIDE + n * 256, lofs4);
                if (narrow) W2[n][k] = w24_ldw2(rs, wp + k * W24_WSTRIDE + 512 + n * 128, lofs2);
            }
    };
    auto park_row6 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int q = 0; q < 4; q++) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][32 + q]) : "v"(Yb[n][q]));
    };
    auto winograd = [&]() __attribute__((always_inline)) {
        unsigned RA[4];
#pragma unroll
        for (int a = 0; a < 4; a++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(RA[a]) : "a"(pk24.a[a]));
        w24_round(RA, rs, wp, wp, lofs4, lofs2, k4 >> 2, pstride, bv, W4, W2, Y);
    };
    const unsigned row5 = wg_parked(pk, 2, 0);
    if constexpr (FIRST) {
        if constexpr (TAPS) w25t_round_direct<true>(row5, rt, tp, lofs4, k4 >> 2, bv, Yb, rs, wp, lofs2, W4, W2);
        else {
            first_steps(false);
            w24_round_direct(row5, rs, wp, lofs4, k4 >> 2, pstride, bv, W4, Yb);
        }
        park_row6();
        if constexpr (!TAPS) first_steps(true);      // (fetched again behind the direct round: held through it they cost it 24 registers)
        winograd();
    } else {
        first_steps(true);
        winograd();
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int q = 0; q < 32; q++) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][q]) : "v"(Y[n][q >> 4][(q >> 2) & 3][q & 3]));
        w25t_round_direct<false>(row5, rt, tp, lofs4, k4 >> 2, bv, Yb, rs, wp, lofs2, W4, W2);
        park_row6();
    }
    __syncthreads();                                 // every wavefront has finished reading the layer's input
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the store offsets are formed here, not kept from the layer's start
#pragma unroll
    for (int n = 0; n < 2; n++) {
        if constexpr (!FIRST) {
#pragma unroll
            for (int q = 0; q < 32; q++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(Y[n][q >> 4][(q >> 2) & 3][q & 3]) : "a"(park[n][q]));
        }
#pragma unroll
        for (int q = 0; q < 4; q++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(Yb[n][q]) : "a"(park[n][32 + q]));
        w24_store_tile(Y[n], 2 * pair + n, relu, act, lane_s & 15, lane_s >> 4);
        wg_store_row6<false>(Yb[n], 2 * pair + n, relu, act, nullptr, lane_s & 15, lane_s >> 4);
    }
}

// The one body of the fused kernel: every layer form but the K split (csrc/convnet_w24k.hip) and the pinned all-F(2x2) stack
// (csrc/convnet_wg.hip) is a branch of the ladder below, picked per layer from the widths and the kernel's relu word as cyl_prepare
// (csrc/cnn_launch.hip) writes it.  To add a form, add a layer function and a branch in front of the forms it replaces; a word without
// the new bit then runs what it ran before.
//   W25_FLAG                    w25_layer_psplit (csrc/convnet_w25.hip): P.wt[l] is the layer's F(2x5) set; 64 or 32 outputs
//   128 outputs                 w25t_layer_pair above with W25T_TAPS or W25T_FIRST, else w24_layer_pair (csrc/convnet_w24.hip)
//   64 outputs, W24K_FLAG       w24p_layer_psplit (csrc/convnet_w24p.hip): P.wt[l] is the layer's F(2x4) set
//   32 outputs, W24K_FLAG       w24a_layer_psplit32 (csrc/convnet_w24a.hip)
//   anything else               wg_layer_msplit / wg_layer_mksplit (csrc/convnet_wg.hip): the F(2x2) form
__device__ __forceinline__ void cyl_net_w25t_body(const float* __restrict__ x, const CylWgParams& P, float* __restrict__ y, float* __restrict__ lds)
{
    float* act = lds;                                // [128][160]
    const int patch = blockIdx.x;
    const int w0 = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    wg_load_input(x, P, act, patch);
    WgAddrPark pk;
    W24AddrPark pk24;
    {
        int lane0 = threadIdx.x & (WAVE - 1);
        asm volatile("" : "+v"(lane0));
        wg_park_addresses(act, lane0 & 15, lane0 >> 4, pk);
        w24_park_addresses(act, lane0 & 15, lane0 >> 4, pk24);
    }
#pragma unroll 1
    for (int l = 0; l < WG_LAYERS; l++) {
        // What depends on the wavefront number is formed per layer, like what depends on the lane number: hoisted out of the layer loop
        // for every layer form at once it spills scalar registers
        int w = w0;
        asm volatile("" : "+s"(w));
        const int cin = P.cin[l], cout = P.cout[l], relu = P.relu[l] & 1;
        const bool f24 = (P.relu[l] & W24K_FLAG) != 0, f25 = (P.relu[l] & W25_FLAG) != 0;
        const bool tp = (P.relu[l] & W25T_TAPS) != 0, df = (P.relu[l] & W25T_FIRST) != 0;
        float* yp = y + (size_t)patch * cout * 140;
        if (f25 && cout == 64) w25_layer_psplit<4, false>(act, nullptr, P.wt[l], P.bias[l], cin, relu, w);
        else if (f25 && l < WG_LAYERS - 1) w25_layer_psplit<2, false>(act, nullptr, P.wt[l], P.bias[l], cin, relu, w);
        else if (f25) w25_layer_psplit<2, true>(act, yp, P.wt[l], P.bias[l], cin, relu, w);
        else if (cout == 128 && tp && df) w25t_layer_pair<true, true>(act, P.wt[l], P.taps[l], P.bias[l], cin, relu, w0, pk, pk24);
        else if (cout == 128 && tp) w25t_layer_pair<true, false>(act, P.wt[l], P.taps[l], P.bias[l], cin, relu, w0, pk, pk24);
        else if (cout == 128 && df) w25t_layer_pair<false, true>(act, P.wt[l], nullptr, P.bias[l], cin, relu, w0, pk, pk24);
        else if (cout == 128) w24_layer_pair(act, P.wt[l], P.bias[l], cin, relu, w0, pk, pk24);
        else if (cout == 64 && f24) w24p_layer_psplit(act, P.wt[l], P.bias[l], cin, relu, w, pk, pk24);
        else if (cout == 64) wg_layer_msplit(act, P.wt[l], P.bias[l], cin, cout, relu, w, pk);
        else if (f24 && l < WG_LAYERS - 1) w24a_layer_psplit32<false>(act, nullptr, P.wt[l], P.bias[l], cin, relu, w, pk, pk24);
        else if (f24) w24a_layer_psplit32<true>(act, yp, P.wt[l], P.bias[l], cin, relu, w, pk, pk24);
        else if (l < WG_LAYERS - 1) wg_layer_mksplit<false>(act, nullptr, P.wt[l], P.bias[l], cin, cout, relu, w, pk);
        else wg_layer_mksplit<true>(act, yp, P.wt[l], P.bias[l], cin, cout, relu, w, pk);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(WG_THREADS, 2) k_cyl_net_w25t(const float* __restrict__ x, CylWgParams P, float* __restrict__ y)
{
    extern __shared__ float lds[];
    cyl_net_w25t_body(x, P, y, lds);
}

// The masked re-run of buf_cylindrical_net_split_safe_w25t, under its own kernel name (see k_cyl_net_wg_rerun)
__global__ void __launch_bounds__(WG_THREADS, 2) k_cyl_net_w25t_rerun(const float* __restrict__ x, CylWgParams P, float* __restrict__ y)
{
    extern __shared__ float lds[];
    if (P.only_if[blockIdx.x] == 0) return;
    cyl_net_w25t_body(x, P, y, lds);
}

// Host helper: filters w [Cout][Cin][3][3] (BN folded) -> the six taps of output row 6, the filter rows a = 0, 1 as they are, in the
// tiling w25t_round_direct streams,
//     out[6 * Cout * Cin] = [pair][k-step][q = 0..2][lk][li][4]
// float 4 q + e = 6 n2 + 3 a + b of lane (lk, li): w[16 (2 pair + n2) + li][4 ks + lk][a][b].  A wavefront's k-step is 768 contiguous
// floats at a wavefront-uniform offset.  No device work.
extern "C" int buf_cyl_row6_tile_taps(const float* w_host, int cout, int cin, float* out_host)
{
    BUF_REQUIRE(w_host && out_host, BUF_EINVAL, "buf_cyl_row6_tile_taps: null argument");
    BUF_REQUIRE(cout > 0 && cin > 0 && cout % 32 == 0 && cin % 4 == 0, BUF_EINVAL, "buf_cyl_row6_tile_taps: widths %d -> %d", cin, cout);
    const int k4 = cin / 4;
    for (int o = 0; o < cout; o++)
        for (int c = 0; c < cin; c++) {
            const float* g = w_host + ((size_t)o * cin + c) * 9;
            const int n = o / 16, lane = (c % 4) * 16 + o % 16;
            float* blk = out_host + ((size_t)(n / 2) * k4 + c / 4) * W25T_STRIDE;
            for (int a = 0; a < 2; a++)
                for (int b = 0; b < 3; b++) {
                    const int f = 6 * (n % 2) + 3 * a + b;
                    blk[(f / 4) * 256 + lane * 4 + f % 4] = g[3 * a + b];
                }
        }
    return BUF_OK;
}
