// A13 -- the one body of the fused fp32 cost net and its kernel pair, behind the layer functions it calls: the first form of every layer
// (csrc/costnet.hip), F(2x4) tiles in layers 2 and 4 and the Winograd layer 6 (csrc/costnet_w24.hip), F(2x4) tiles in layer 1 and the hybrid
// layer 3 (csrc/costnet_w24b.hip).  Every layer that has a second form is switched by its filter set in CostNetParams::f24: a null set runs
// the first form from the same buffer with the same arguments, so five null sets are the F(2x2) net throughout and the entry points
// without sets, with three and with five (csrc/cnn_launch.hip) are one kernel.
#include "common.h"

#ifdef CV_STAMP
__device__ long long* cv_stamp_ptr;       // development build (-DCV_STAMP): s_memtime of wavefront 0 at the phase boundaries
#define CV_STAMP_AT(SLOT) if (threadIdx.x == 0) cv_stamp_ptr[(size_t)blockIdx.x * 16 + (SLOT)] = __builtin_amdgcn_s_memtime();
#else
#define CV_STAMP_AT(SLOT)
#endif

__device__ __forceinline__ void cost_net_body(const float* __restrict__ s_eq, const float* __restrict__ t_eq, const CostNetParams& P,
                                              float* __restrict__ ind_out, float* __restrict__ lds)
{
    const float* const* f24 = P.f24;
    // lds: ONE buffer of CV_BUF floats (75 KB): two workgroups per CU
    float* bufA = lds;                       // every map from layer 1 on (layers 2..6 rewrite it in place)
    float* bufB = lds;                       // phase A: the maps of the separated layer 0 and the row chunks live here first
    float* SP = bufB + CVA_SP;
    float* TP = bufB + CVA_TP;
    float* SM = bufB + CVA_SM;
    float* TB = bufB + CVA_TB;
    const int match = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), li = lane & 15, lk = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);        // wavefront-uniform for the compiler too (scalar weight offsets)
    {   // both maps, transposed on the way in: global [c][k][l] -> LDS [k][l][c]; S with its two wrap-around columns per side
        const float* a = s_eq + (P.s_rows ? (size_t)P.s_rows[match] * P.row_floats + P.skip_floats : (size_t)match * 3200);
        const float* b = t_eq + (P.t_rows ? (size_t)P.t_rows[match] * P.row_floats + P.skip_floats : (size_t)match * 3200);
        for (int i = tid; i < 800; i += CV_THREADS) {
            const int c = i / 25, rem = i - c * 25, k = rem / 5, l0 = (rem - k * 5) * 4;
            // (read once: streamed past the L2, which is for the 2.9 MB of filters every workgroup walks)
            const cvx4 sv = __builtin_nontemporal_load(reinterpret_cast<const cvx4*>(a + c * P.chan_floats + rem * 4));      // 100 contiguous floats per channel
            const cvx4 tv = __builtin_nontemporal_load(reinterpret_cast<const cvx4*>(b + c * P.chan_floats + rem * 4));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int l = l0 + q;
                SP[(k * 24 + l + 2) * CV_C32 + c] = sv[q];
                if (l >= 18) SP[(k * 24 + l - 18) * CV_C32 + c] = sv[q];
                if (l < 2) SP[(k * 24 + l + 22) * CV_C32 + c] = sv[q];
                TP[(k * 20 + l) * CV_C32 + c] = tv[q];
            }
        }
    }
    __syncthreads();
    CV_STAMP_AT(0)

    // ---- phase A.1: the two small GEMMs of the separated layer 0; wave w owns M-tile w (16 positions), both N-tiles ----
    {
        const float b0v[2] = { P.bias[0][li], P.bias[0][16 + li] };
        int ms = w * 16 + li, mt = ms;
        ms = ms < 60 ? ms : 59;                              // padding rows recompute the last position (never stored)
        mt = mt < 54 ? mt : 53;
        SLoader LS;
        LS.base = SP + ((ms / 20) * 24 + ms % 20) * CV_C32 + lk * 4;
        TLoader LT;
        LT.base = TP + ((mt / 18) * 20 + mt % 18) * CV_C32 + lk * 4;
        cvx4 accS[1][2] = { { (cvx4){ 0.f, 0.f, 0.f, 0.f }, (cvx4){ 0.f, 0.f, 0.f, 0.f } } };
        cvx4 accT[1][2] = { { (cvx4){ 0.f, 0.f, 0.f, 0.f }, (cvx4){ 0.f, 0.f, 0.f, 0.f } } };
        cv_gemm_static<1, 2, 4, 30>(accS, LS, P.wt[0] + (size_t)lane * 4, 2);
        cv_gemm_static<1, 2, 4, 18>(accT, LT, P.wt[0] + (size_t)30 * 2 * 256 + (size_t)lane * 4, 2);
        // C/D layout: lane holds channel n = 16u + li at the four positions m = 16w + 4lk + r
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = w * 16 + lk * 4 + r;
                if (m < 60) SM[m * CV_C32 + u * 16 + li] = accS[0][u][r];
                if (m < 54) TB[m * CV_C32 + u * 16 + li] = b0v[u] - accT[0][u][r];
            }
    }
    __syncthreads();                         // SM/TB complete; SP/TP dead from here on (the chunk buffer XC takes their place)
    CV_STAMP_AT(1)

    // ---- phase A.2: layer 1 in the Winograd domain.  Its 3 x 3 x 3 filter collapses k' (3 -> 1), so it is a 3 x 3 correlation over
    // (n', l') with the three k' planes as input channels (96).  With a set: F(2x4) tiles, one k' plane at a time (cw24b_layer1).
    // Without: 8 x 8 tiles of 2 x 2 outputs.  The 124 KB layer-0 map never exists: four chunks of six rows n' = 4j .. 4j+5 (two tile rows = one M-tile of 16 tiles) are formed channel-major one after
    // the other.  Wavefront (p, kh) owns the N-tile PAIR p over half kh of K (48 channels): one input transform feeds 8 MFMAs.  The two
    // K halves of a pair share the stores (kh = 0: chunks 0, 1; kh = 1: chunks 2, 3): the partial sums of a chunk go from the half
    // that does not store it to the one that does, which holds its 2 x 32 output registers until the last chunk has been read.
    // 64 tile rows x 16 components x 96 channels = 0.44 of the direct form's matrix instructions (3 456 -> 1 536 per wavefront).
    if (f24[3] != nullptr) {
        cw24b_layer1(lds, f24[3], P.bias[1], w);
        CV_STAMP_AT(2)
    } else {
        int lane_ = threadIdx.x & (WAVE - 1);
        asm volatile("" : "+v"(lane_));
        const int li_ = lane_ & 15, lk_ = lane_ >> 4;
        const int p_ = w & 1, kh = w >> 1;
        float* XC = bufB + CVA_XC;
        constexpr unsigned KSTEP = 16u * CW_CSX;
        const __amdgpu_buffer_rsrc_t rs = wg_weights(P.wt[1]);
        const unsigned wp = (unsigned)p_ * (96 * 512) + (unsigned)(12 * kh) * 512;      // [pair][i 0..3][k-step 0..23][n2][lane][j]
        const unsigned lofs = lane_ * 16;
        unsigned RA[3][4];
        {
            const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)XC + (unsigned)(12 * kh) * KSTEP;
#pragma unroll
            for (int a = 0; a < 4; a++) RA[0][a] = RA[1][a] = RA[2][a] = base + 4u * (unsigned)(lk_ * CW_CSX + (2 * (li_ >> 3) + a) * CW_RSX + 2 * (li_ & 7));
        }
        const float* bl = kh ? nullptr : P.bias[1] + p_ * 32 + lk_ * 4;               // the bias rides in the lower K half
        wgf4 W[2][2];
        wg_first_weights<2, 0, 2>(rs, wp, lofs, 512, W);
        // kh = 0 stores chunks 0, 1 and kh = 1 chunks 2, 3: after a chunk's round the other half hands its 8 quads over through the
        // 16 KB between the chunk buffer and the layer-0 maps, before the barrier that ends the chunk; the owner adds them behind it
        wgf4* slot = reinterpret_cast<wgf4*>(bufB + CVA_XCH) + (size_t)p_ * 8 * WAVE + lane_;
        wgf4 Yown[2][2][3][2][2];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            form_rows_cm(XC, SM, TB, 4 * j);
            __syncthreads();
            wgf4 Yt[2][3][2][2];
            wg_round<2, 0, 1, KSTEP, true>(RA, rs, wp, wp, lofs, 3, 512, 24u * 512u, bl, W, Yt);
            const bool own = (j < 2) == (kh == 0);
            if (!own) {
#pragma unroll
                for (int q = 0; q < 8; q++) slot[q * WAVE] = Yt[q >> 2][0][(q >> 1) & 1][q & 1];
            }
            __syncthreads();                 // the chunk may be overwritten; the partial sums handed over are in place
            if (own) {
#pragma unroll
                for (int q = 0; q < 8; q++) Yown[j & 1][q >> 2][0][(q >> 1) & 1][q & 1] = Yt[q >> 2][0][(q >> 1) & 1][q & 1] + slot[q * WAVE];
            }
        }
        // (the last take and the next barrier: the map below covers the slots)
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 2; jj++)
#pragma unroll
            for (int n = 0; n < 2; n++)
                cw_store_tile<18, 2, 16, CW_CS1, false>(Yown[jj][n][0], 2 * kh + jj, 2 * p_ + n, bufA, li_, lk_);
        __syncthreads();
        CV_STAMP_AT(2)
    }
    // ---- phase B: layers 2..6 rewrite the buffer in place; the three tiny last layers hop through its free parts -----------
    //                                 in: size rows stride | tile rows per M-tile | Cin | N-tiles, M-tiles per wavefront | out
    if (f24[0] != nullptr) {                 // wavefront (pair, M-tile): M-tile 0 holds the tile rows 0..3, M-tile 1 the rows 4..6
        cw24_zero_spare<64, CW_CS1, 256>(bufA);
        __syncthreads();
        cw24_layer<16, 16, CW_CS1, 4, 4, 64, 14, CW_CS2>(bufA, f24[0], P.bias[2], w & 1, w >> 1);
    } else
        cw_layer<16, 16, CW_CS1, 2, 64, 2, 2, 0, 14, CW_CS2, false>(bufA, P.wt[2], P.bias[2], w & 1, 2 * (w >> 1));   // 16x16 -> 14x14, 64 ch
    __syncthreads();
    CV_STAMP_AT(3)
    if (f24[4] != nullptr)                   // wavefront w owns pair w: 5 x 3 F(2x4) tiles (rows 0..9), then the F(2x2) tile row 5 (rows 10, 11)
        cw24b_layer3(bufA, f24[4], P.wt[3], P.bias[3], w);
    else
        cw_layer<14, 14, CW_CS2, 2, 64, 2, 2, 1, 12, CW_CS3, false>(bufA, P.wt[3], P.bias[3], w, 0);              // -> 12x12, 128 ch
    __syncthreads();
    CV_STAMP_AT(4)
    if (f24[1] != nullptr) {                 // wavefront w owns pair w over the one M-tile of 5 x 3 tiles
        cw24_zero_spare<128, CW_CS3, 144>(bufA);
        __syncthreads();
        cw24_layer<12, 12, CW_CS3, 3, 5, 128, 12, CW_CS3>(bufA, f24[1], P.bias[4], w, 0);
    } else
        cw_layer<12, 12, CW_CS3, 3, 128, 2, 2, 0, 12, CW_CS3, false>(bufA, P.wt[4], P.bias[4], w, 0);             // -> 10x10 (rows of 12)
    __syncthreads();
    CV_STAMP_AT(5)
    if (f24[2] != nullptr) {
        cw_layer<10, 12, CW_CS3, 4, 128, 1, 1, 0, 8, CW_CS5, false>(bufA, P.wt[5], P.bias[5], w, 0);              // -> 8x8, channel-major
        __syncthreads();
        CV_STAMP_AT(6)
        cw_layer<8, 8, CW_CS5, 3, 64, 1, 1, 0, 0, CV_C64, true>(bufA, f24[2], P.bias[6], w, 0);                   // -> 6x6, position-major
    } else {
        cw_layer<10, 12, CW_CS3, 4, 128, 1, 1, 0, 0, CV_C64, true>(bufA, P.wt[5], P.bias[5], w, 0);               // -> 8x8, position-major
        __syncthreads();
        CV_STAMP_AT(6)
        cv_conv_layer<3, 1, 64, 64, 8, 3, true>(bufA, bufA, P.wt[6], P.bias[6], w, true);        // -> 6x6 (36 x 68 floats)
    }
    __syncthreads();
    CV_STAMP_AT(7)
    float* hop1 = lds + 4096;
    float* hop2 = lds + 8192;
    float* hop3 = lds + 12288;
    if (w < 2) cv_conv_layer<1, 1, 64, 32, 6, 3, false>(bufA, hop1, P.wt[7], P.bias[7], w, true);    // -> 4x4
    __syncthreads();
    if (w < 2) cv_conv_layer<1, 1, 32, 32, 4, 3, false>(hop1, hop2, P.wt[8], P.bias[8], w, true);    // -> 2x2
    __syncthreads();
    if (w < 2) cv_conv_layer<1, 1, 32, 32, 2, 2, false>(hop2, hop3, P.wt[9], P.bias[9], w, false);   // -> 1x1, 20 (+12 zero) logits
    __syncthreads();
    CV_STAMP_AT(8)
    if (w == 0) {                            // softmax over the 20 logits, expected index (BUFFER.py:63-65)
        float v = lane < 20 ? hop3[lane] : -3.4e38f;               // the 1x1 map: position 0, channels 0..19
        float mx = v;
        for (int d = WAVE / 2; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, WAVE));
        float e = lane < 20 ? expf(v - mx) : 0.f;
        float se = e, sw = e * (float)lane;
        for (int d = WAVE / 2; d > 0; d >>= 1) { se += __shfl_xor(se, d, WAVE); sw += __shfl_xor(sw, d, WAVE); }
        if (lane == 0) ind_out[match] = sw / se;
    }
}

// The kernel keeps the name it had as the largest of three: profiles and A/B documents written before the smaller two were retired name it.
__global__ void __launch_bounds__(CV_THREADS, 2) k_cost_net_w24b(const float* __restrict__ s_eq, const float* __restrict__ t_eq, CostNetParams P,
                                                             float* __restrict__ ind_out)
{
    extern __shared__ float lds[];
    cost_net_body(s_eq, t_eq, P, ind_out, lds);
}

// The masked re-run of the buf_cost_volume_net_split_safe family (matches the split-f16 kernel flagged): its own kernel name, see
// k_cyl_net_wg_rerun.
__global__ void __launch_bounds__(CV_THREADS, 2) k_cost_net_w24b_rerun(const float* __restrict__ s_eq, const float* __restrict__ t_eq, CostNetParams P,
                                                                   float* __restrict__ ind_out)
{
    extern __shared__ float lds[];
    if (P.only_if[blockIdx.x] == 0) return;
    cost_net_body(s_eq, t_eq, P, ind_out, lds);
}
