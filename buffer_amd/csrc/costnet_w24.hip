// A13 -- the F(2x4) layer of the fused fp32 cost net (cw24_layer): the second form of layers 2 and 4, which cost_net_body
// (csrc/costnet_body.hip) runs where CostNetParams::f24[0] / f24[1] hold the layer's F(2x4) set.  With the Winograd form of layer 6
// (f24[2]: cw_layer of csrc/costnet.hip on an F(2x2) set) these are the three forms the entry points *_w24 added:
//
//   layer 2 (64 -> 64, 16 x 16 -> 14 x 14)    F(2x4, 3x3) tiles of 2 rows x 4 columns: 7 x 4 = 28 tiles in two M-tiles (16 + 12),
//                                             2 x 24 = 48 matrix instructions per (k-step, N-tile) instead of the 64 of F(2x2)
//   layer 4 (128 -> 128, 12 x 12 -> 10 x 10)  F(2x4): 5 x 3 = 15 tiles in ONE M-tile, 24 instead of 32
//   layer 6 (64 -> 64, 8 x 8 -> 6 x 6)        F(2x2) on cw_layer: 3 x 3 = 9 tiles in one M-tile, 16 instead of the 27 of the direct form;
//                                             layer 5 then leaves its 8 x 8 map channel-major, [64][CW_CS5]
// 30 384 -> 26 608 matrix instructions per match.  Layers 2 and 4 run the pair form of the descriptor CNN's 128-output layers (w24_round /
// w24_pass of csrc/convnet_w24.hip: a wavefront owns an N-tile pair, four row-component passes of 12 MFMAs per k-step, A4^T folded after
// each pass, the bias in column component 1) over the unpadded channel-major maps of this kernel.
//
// The window of a tile is 4 rows x 6 consecutive words from column 4 tx (an even word: three ds_read_b64 per row).  The LAST tile column
// reads two words past its row -- the first two of the next row, and behind the last row the first two of the channel's 16 spare words
// (CS - rows x row length), which are zeroed before the layer's first read.  Those words only meet the tile's output columns 14, 15
// (layer 2) / 10, 11 (layer 4), which are dropped; they are finite and of the map's scale, so the round-off they add to the kept
// columns through A4^T is that of any other window word.
//
// Every layer is switched by its filter set: a null set runs the layer's F(2x2) form (layer 6: the direct form) of csrc/costnet.hip.
#include "common.h"

// the 16 spare words behind the HIN rows of every channel of the map [C][CS]
template <int C, int CS, int USED>
__device__ __forceinline__ void cw24_zero_spare(float* __restrict__ map)
{
    static_assert(CS - USED == 16, "16 spare words per channel");
    for (int i = threadIdx.x; i < C * 16; i += CV_THREADS) map[(i >> 4) * CS + USED + (i & 15)] = 0.f;
}

// One F(2x4) layer over the map in `map` (HIN x HIN, rows of RS, channel stride CS), rewritten in place as [Cout][CSO] with rows of RSO:
// this wavefront's N-tile pair `pair` over M-tile t, which holds TYPM tile rows of NTX tiles.  Idle lanes recompute tile (0, 0).
template <int HIN, int RS, int CS, int NTX, int TYPM, int CIN, int RSO, int CSO>
__device__ __forceinline__ void cw24_layer(float* __restrict__ map, const float* __restrict__ wt, const float* __restrict__ bias, int pair, int t)
{
    constexpr int WOUT = HIN - 2, NTY = WOUT / 2;
    static_assert(NTX * TYPM <= 16 && 4 * NTX >= WOUT && 4 * (NTX - 1) + 2 <= WOUT && RS % 2 == 0 && CS % 2 == 0 && RSO % 2 == 0 && CSO % 2 == 0 && CIN % 16 == 0, "");
    static_assert((HIN - 1) * RS + 4 * (NTX - 1) + 6 <= CS, "the last window stays inside the channel");
    constexpr unsigned KSTEP = 16u * CS;
    constexpr int k4 = CIN / 4;
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int lk = lane >> 4;
    const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)map;
    unsigned RA[4];
    {
        const int li = lane & 15, q = li / NTX;
        int ty = t * TYPM + q, tx = li - q * NTX;
        if (!(q < TYPM && ty < NTY)) { ty = 0; tx = 0; }
#pragma unroll
        for (int a = 0; a < 4; a++) RA[a] = base + 4u * (unsigned)(lk * CS + (2 * ty + a) * RS + 4 * tx);
    }
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
    w24_round<false, KSTEP>(RA, rs, wp, wp, lofs4, lofs2, k4 >> 2, pstride, bv, W4, W2, Y);
    __syncthreads();                         // every wavefront has finished reading the map
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));         // the store offsets are formed here, not kept from the layer's start
    const int li = lane_s & 15, q = li / NTX, tx = li - q * NTX, ty = t * TYPM + q;
    if (!(q < TYPM && ty < NTY)) return;
    const bool wide = 4 * tx + 2 < WOUT;     // the tile's output columns 2, 3 exist
#pragma unroll
    for (int n = 0; n < 2; n++) {
        float* p = map + ((2 * pair + n) * 16 + (lane_s >> 4) * 4) * CSO + 2 * ty * RSO + 4 * tx;
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float* d = p + r * CSO + u * RSO;
                *reinterpret_cast<wgf2*>(d) = (wgf2){ fmaxf(Y[n][u][0][r], 0.f), fmaxf(Y[n][u][1][r], 0.f) };
                if (wide) *reinterpret_cast<wgf2*>(d + 2) = (wgf2){ fmaxf(Y[n][u][2][r], 0.f), fmaxf(Y[n][u][3][r], 0.f) };
            }
    }
}
