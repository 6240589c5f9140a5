// A11 dense part -- k_cyl_net_w24k: the F(2x4, 3x3) form of the 128-output layers (csrc/convnet_w24.hip) in the layers of 64 output
// channels as well, where Cin is a multiple of 64 (the released stack: 64 -> 64 twice and 128 -> 64; 256 of its 736 (k-step, N-tile) units, at
// 30 instead of 38 matrix instructions each: 22 848 per patch = 38 x 96 + 30 x 640 against 24 896).
//
// One F(2x4) M-tile carries the whole map, so the M split of wg_layer_msplit has nothing to split; the four wavefronts keep the
// N-tile-pair form (one input transform feeds 12 MFMAs) by splitting K: wavefront w owns the N-tile pair w & 1 over the K half w >> 1
// and runs w24_round and w24_round_direct as they are over its half -- weights from k-step half * (k4 / 2) of the pair's set on, the
// window rows that many k-steps further up the channel axis.  The bias rides in the lower half.
//
// The exchange is balanced: of the pair's two N-tiles, wavefront (pair, half) RECEIVES N-tile `half` and DONATES the other, 32 + 4
// floats per lane each way (nine 16-byte LDS writes, nine reads and 36 adds per wavefront and layer).  The receiver adds, applies the
// ReLU and stores with w24_store_tile / wg_store_row6.
//
// The exchange area: the rows of the channels 64..127, words 0..143 of each (wavefront w writes the 16 rows from channel 64 + 16 w on:
// lane (row = lane >> 2, quarter = lane & 3) has nine float4 from word 36 quarter on).  The four zero words of these channels
// (WG_ZERO..WG_ZERO + 3) are written once per kernel and a LATER layer with 128 input channels reads them: they are not touched, nor
// are the two dump words.  With Cin = 64 the area is free while the layer computes -- the partial sums are written before the in-place
// barrier and read behind it, one barrier as in every other form; with Cin = 128 it is input until that barrier: barrier, write,
// a second barrier, read.  Both kinds of held outputs wait in accumulation registers, as in w24_layer_pair.
// (The lane stride of 36 words makes the nine ds_write_b128 / ds_read_b128 of the exchange bank-conflicted; at nine quads per wavefront
// and layer this was left as it is and has not been measured on its own.)
//
// Opt-in: bit 2 of relu_host[l] (BUF_CYL_F24K) on a layer with 64 output channels and Cin % 64 == 0 says that the layer's buffer holds
// the F(2x4) set (buf_winograd_f24_tile_weights) behind the F(2x2) set; the bit-1 rule of the 128-output layers holds beside it.  Stacks
// without bit 2 never come here.
#include "common.h"

#define W24K_FLAG BUF_CYL_F24K
#define W24K_XCH_C 64          // first channel row of the exchange area
#define W24K_XCH_QUADS 9       // float4 per lane: 2 x 4 of the Winograd round, one of row 6

// One N-tile's parked partial outputs (accumulation registers) back into nine quads
__device__ __forceinline__ void w24k_unpark(const float (&parked)[4 * W24K_XCH_QUADS], wgf4 (&Q)[W24K_XCH_QUADS])
{
#pragma unroll
    for (int q = 0; q < 4 * W24K_XCH_QUADS; q++) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(Q[q >> 2][q & 3]) : "a"(parked[q]));
}

__device__ __forceinline__ void w24k_layer_ksplit(float* __restrict__ act, const float* __restrict__ wt, const float* __restrict__ bias, int cin, int relu,
                                                  int w, const WgAddrPark& pk, const W24AddrPark& pk24)
{
    // (the dump words of the input channels: see w24_layer_pair)
    act[(threadIdx.x >> 1) * WG_CS + WG_ZERO + 4 + (threadIdx.x & 1)] = 0.f;
    __syncthreads();
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const int pair = w & 1, half = w >> 1;
    const int k4 = cin >> 2, kn = k4 >> 1;
    const unsigned kofs = (unsigned)(half * kn) * WG_KSTEP;                // this half's first k-step in the activation buffer
    unsigned RA[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(RA[a]) : "a"(pk24.a[a]));
        RA[a] += kofs;
    }
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned pstride = (unsigned)(k4 * W24_WSTRIDE);
    const unsigned wp = (unsigned)pair * 4 * pstride + (unsigned)(half * kn) * W24_WSTRIDE;     // [pair][i][k-step][...]
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8;
    const float* bv = half ? nullptr : bias + (2 * pair) * 16 + lk * 4;
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
    float park[2][36];                               // accumulation registers: both N-tiles' partial outputs, as in w24_layer_pair
    w24_round<true>(RA, rs, wp, wp, lofs4, lofs2, kn >> 2, pstride, bv, W4, W2, Y);
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int q = 0; q < 32; q++) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][q]) : "v"(Y[n][q >> 4][(q >> 2) & 3][q & 3]));
    // (row 6's window address and the bias pointer are formed here: held through the Winograd round they cost it two registers)
    const unsigned row5 = wg_parked(pk, 2, 0) + kofs;
    int lane_d = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_d));
    const float* bvd = half ? nullptr : bias + (2 * pair) * 16 + (lane_d >> 4) * 4;
    wgf4 Yb[2];
    w24_round_direct<true>(row5, rs, wp, lofs4, kn >> 2, pstride, bvd, W4, Yb);
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int q = 0; q < 4; q++) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[n][32 + q]) : "v"(Yb[n][q]));
    if (cin > W24K_XCH_C) __syncthreads();           // the exchange area is this layer's input: every wavefront has finished reading it
    // N-tile `half` of the pair is finished here, the other one handed over.  Which parked set is which is a wavefront-uniform branch
    // around the register reads (72 selects on the parked values otherwise).
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the exchange and store offsets are formed here, not kept from the layer's start
    const int xofs = (W24K_XCH_C + (lane_s >> 2)) * WG_CS + (lane_s & 3) * (4 * W24K_XCH_QUADS);
    wgf4 Q[W24K_XCH_QUADS];
    if (half) w24k_unpark(park[0], Q);
    else w24k_unpark(park[1], Q);
    wgf4* mine = reinterpret_cast<wgf4*>(act + xofs + 16 * w * WG_CS);
#pragma unroll
    for (int q = 0; q < W24K_XCH_QUADS; q++) mine[q] = Q[q];
    __syncthreads();                                 // the partial sums are in place AND every wavefront has finished reading the input
    if (half) w24k_unpark(park[1], Q);
    else w24k_unpark(park[0], Q);
    const wgf4* theirs = reinterpret_cast<const wgf4*>(act + xofs + 16 * (w ^ 2) * WG_CS);
    wgf4 Yk[2][4];
#pragma unroll
    for (int q = 0; q < W24K_XCH_QUADS; q++) {
        Q[q] += theirs[q];
        if (q < 8) Yk[q >> 2][q & 3] = Q[q];
    }
    w24_store_tile(Yk, 2 * pair + half, relu, act, lane_s & 15, lane_s >> 4);
    wg_store_row6<false>(Q[8], 2 * pair + half, relu, act, nullptr, lane_s & 15, lane_s >> 4);
}

// The body of the K-split stacks, the one form cyl_net_w25t_body (csrc/convnet_w25t.hip) does not hold: P.relu[l] keeps bit 2
// (W24K_FLAG) beside the ReLU bit
__device__ __forceinline__ void cyl_net_w24k_body(const float* __restrict__ x, const CylWgParams& P, float* __restrict__ y, float* __restrict__ lds)
{
    float* act = lds;                                // [128][160]
    const int patch = blockIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
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
        const int cin = P.cin[l], cout = P.cout[l], relu = P.relu[l] & 1;
        if (cout == 128) w24_layer_pair(act, P.wt[l], P.bias[l], cin, relu, w, pk, pk24);
        else if (cout == 64 && (P.relu[l] & W24K_FLAG)) w24k_layer_ksplit(act, P.wt[l], P.bias[l], cin, relu, w, pk, pk24);
        else if (cout == 64) wg_layer_msplit(act, P.wt[l], P.bias[l], cin, cout, relu, w, pk);
        else if (l < WG_LAYERS - 1) wg_layer_mksplit<false>(act, nullptr, P.wt[l], P.bias[l], cin, cout, relu, w, pk);
        else wg_layer_mksplit<true>(act, y + (size_t)patch * cout * 140, P.wt[l], P.bias[l], cin, cout, relu, w, pk);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(WG_THREADS, 2) k_cyl_net_w24k(const float* __restrict__ x, CylWgParams P, float* __restrict__ y)
{
    extern __shared__ float lds[];
    cyl_net_w24k_body(x, P, y, lds);
}

// The masked re-run of buf_cylindrical_net_split_safe, under its own kernel name (see k_cyl_net_wg_rerun)
__global__ void __launch_bounds__(WG_THREADS, 2) k_cyl_net_w24k_rerun(const float* __restrict__ x, CylWgParams P, float* __restrict__ y)
{
    extern __shared__ float lds[];
    if (P.only_if[blockIdx.x] == 0) return;
    cyl_net_w24k_body(x, P, y, lds);
}
