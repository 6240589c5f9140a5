// A13 -- CostVolume + CostNet (models/BUFFER.py:37-66, models/patchnet.py:88-147) as ONE fused fp32-MFMA kernel.
//
// Reference: gather the 20 circular azimuth shifts of the source map, subtract the target map
// ([M,32,20,5,20] = 256 KB per match), ten unpadded Conv3d (3x3x3, 3x3x3, 7 x (3,1,3), (2,1,2)) with
// BatchNorm(affine=False)+ReLU, softmax over the 20 logits, expected index.
//
// Here one workgroup owns one match and the cost volume is never built.  Layer 0 is LINEAR in
//     cost[c][n][k][l] = S[c][k][(l-n) mod 20] - T[c][k][l],
// so its pre-activation separates exactly (only fp32 re-association, <= 1e-6) into
//     out0[o][n'][k'][l'] = b[o] + Sterm[o][k'][(l'-n') mod 20] - Tterm[o][k'][l'],
//     Sterm[o][k'][j]  = sum_{c,dk,e}  Ws[o][c][dk][e]  S[c][k'+dk][(j+e) mod 20],   Ws[..][e] = sum_{dl-dn=e} W0[o][c][dn][dk][dl]
//     Tterm[o][k'][l'] = sum_{c,dk,dl} Wt[o][c][dk][dl] T[c][k'+dk][l'+dl],          Wt        = sum_dn      W0[o][c][dn][dk][dl]
// (the S-term of output (n',k',l') depends on (k', (l'-n') mod 20) only: 60 positions, K = 480; the T-term does not depend
// on n': 54 positions, K = 288): 1.4 M MAC instead of the 26.9 M of the dense layer 0.  The two small maps are two MFMA GEMMs;
// a layer-0 row is then relu(Smap + (b - Tmap)) formed by VALU, six rows (n') at a time into an LDS chunk that layer 1
// consumes at once, so the 124 KB layer-0 activation never exists either.  Layers 2..6 rewrite ONE 80 KB LDS buffer in place
// (two workgroups per CU).  Layers 1..5 are unpadded 3 x 3 correlations over (n, l) -- layer 1 collapses k' (3 -> 1): its three
// k' planes are 96 input channels; 18 -> 16 -> 14 -> 12 -> 10 -> 8; together 92 % of the kernel's matrix instructions in the
// direct form -- and run in the Winograd F(2x2, 3x3) domain on the pass machinery of csrc/convnet_wg.hip (phase A.2 of cost_net_body and cw_layer
// below: 0.49 of their direct-form MFMAs).  (Layer 1 in the direct form -- three-row chunks, a sliding window of accumulator
// rows -- executed 0.83 of the matrix peak and was 14 % slower.)
// All GEMMs run on v_mfma_f32_16x16x4_f32 (fp32), weights (BN folded; [K][Cout] MFMA-tiled, or G g G^T in the Winograd tiling)
// stream from L2.
// FLOP accounting: bench.py credits the DENSE algorithmic count of SURVEY 8d (0.160 GFLOP/match); executed: 0.0519 GFLOP.
//
// The LDS maps of the direct-form layers are POSITION-major, [position][channels + 4]: the four k-steps of a 16-channel group that a lane feeds
// to the MFMA A operand (channels 16g + 4lk + 0..3 at its position) are one 16-byte ds_read_b128, and the +4 padding
// (row stride = 4 mod 32 banks) keeps eight neighbouring positions on distinct bank quads.  With one wavefront per SIMD
// the number of memory instructions per MFMA, not their bytes, sets the MFMA duty: 1 LDS + 1-2 global loads per group.
//
// This file holds the FIRST form of every layer: the GEMMs and loaders of the separated layer 0, the direct-form layer (cv_conv_layer:
// layers 6..9) and the F(2x2) Winograd layer (cw_layer: layers 2..5, and layer 6 behind a channel-major layer 5).  The cheaper tilings
// that a filter set switches on are in csrc/costnet_w24.hip (layers 2, 4: F(2x4)) and csrc/costnet_w24b.hip (layers 1, 3); the one body
// that runs every form, cost_net_body, and the kernel pair are behind all three in csrc/costnet_body.hip.
#include "common.h"

#define CV_THREADS 256
#define CV_BUF 20480              // floats of the one LDS buffer (largest map: 128 channels x 160, the 12 x 12 map of layers 3 / 4)
#define CV_LAYERS 10
#define CV_C32 36                 // position-row strides (floats) of maps with 32 / 64 / 128 channels
#define CV_C64 68
#define CV_C128 132

typedef float cvx4 __attribute__((ext_vector_type(4)));

// A group's operand loads are woven into the previous group's MFMAs: after every MFMA up to 4 VALU/SALU and the
// group's memory instructions spread evenly (NMEM over NMFMA, rounded up).
#define CV_SCHED_TAIL(NMFMA, NMEM)                                                      \
    _Pragma("unroll") for (int i_ = 0; i_ < (NMFMA); i_++) {                            \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x006, 4, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x120, ((NMEM) + (NMFMA) - 1) / (NMFMA), 0); \
    }
typedef const __attribute__((address_space(1))) cvx4* cv_gptr;     // global (not flat) 16-byte weight loads

struct CostNetParams {
    const float* wt[CV_LAYERS];    // [K][Cout] in the MFMA tiling described at cv_gemm_static; K ordering per layer below
    const float* bias[CV_LAYERS];
    // gathered form (buf_cost_volume_net_gather): match i reads rows s_rows[i] / t_rows[i] of a full [rows,32,ele_n,20] map and
    // takes its elevation rows 1..5 (models/BUFFER.py:291-292) inside the kernel; null rows = dense [m,32,5,20] inputs
    const long long* s_rows;
    const long long* t_rows;
    int row_floats, chan_floats, skip_floats;
    const int* only_if;            // nullable: workgroup i runs only if only_if[i] != 0 (the fp32 re-run of buf_cost_volume_net_split_safe)
    // nullable filter sets, one per layer form that has a cheaper tiling; a layer whose set is null runs its first form from wt[]:
    //   f24[0], f24[1]  F(2x4) sets of layers 2 and 4 (buf_winograd_f24_tile_weights)       csrc/costnet_w24.hip
    //   f24[2]          F(2x2) set of layer 6 (buf_winograd_tile_filters, group 1)
    //   f24[3], f24[4]  F(2x4) sets of layers 1 and 3                                       csrc/costnet_w24b.hip
    const float* f24[5];
};

// ---- tile GEMM: acc[t][u] += sum over groups of 4 k-steps ---------------------------------------------------------
// Loader::load(a, g): fills a[p][t] (p = k-step inside the group, t = M-tile) for group g.
// Weights come TILED for the MFMA B operand: block (group g of 16 K-rows, N-tile n) = 256 floats laid out
// [lane = lk*16 + li][p], so the four B values a lane needs for the four k-steps of a group are ONE 16-byte load and a
// wavefront reads 1 KB contiguously; blocks ordered [g][n].  wl = tiled + (nt0*64 + lane)*4.  K-row of (g, p, lk) is
// 16g + 4lk + p: k-step p of a group takes channel 4lk + p from every lane quarter, matching the A loads above.
// Fully unrolled variant for a compile-time group count: every tap/channel-group index, LDS offset and weight
// offset folds to an immediate, so a group costs no address arithmetic at all (the operand loads of the small
// layer-0/1 tiles otherwise take as many issue cycles as their 4-8 MFMAs).
template <int MT, int NT, int D, int TOTAL, typename Loader>
__device__ __forceinline__ void cv_gemm_static(cvx4 (&acc)[MT][NT], Loader& L, const float* __restrict__ wl, int ntot)
{
    float a[D][4][MT], b[D][4][NT];
#define CVS_LOAD(SLOT, G)                                                                                 \
    {                                                                                                     \
        /* one address per group, pinned here (not hoisted out of the caller's loop) and typed as global  \
           memory so that the loads stay global_load (in-order vmcnt), not flat_load */                   \
        cv_gptr wg_ = (cv_gptr)(wl + (size_t)(G) * ntot * 256);                                           \
        asm volatile("" : "+v"(wg_));                                                                     \
        _Pragma("unroll") for (int u = 0; u < NT; u++) {                                                  \
            const cvx4 bv_ = wg_[u * 64];                                                                 \
            _Pragma("unroll") for (int p = 0; p < 4; p++) b[SLOT][p][u] = bv_[p];                         \
        }                                                                                                 \
        L.load(a[SLOT], (G));                                                                             \
    }
#pragma unroll
    for (int i = 0; i < D - 1; i++) CVS_LOAD(i, i)
#pragma unroll
    for (int g = 0; g < TOTAL; g++) {
        __builtin_amdgcn_sched_barrier(0);
        if (g + D - 1 < TOTAL) CVS_LOAD((g + D - 1) % D, g + D - 1)
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int t = 0; t < MT; t++)
#pragma unroll
                for (int u = 0; u < NT; u++)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g % D][p][t], b[g % D][p][u], acc[t][u], 0, 0, 0);
        CV_SCHED_TAIL(4 * MT * NT, MT + NT)
    }
#undef CVS_LOAD
}

// ---- phase A operand loaders (every map position-major with a 36-float row: 32 channels + 4 padding) ---------------
// LDS regions of phase A inside the bufB half (floats):
#define CVA_SP 0          // [5][24][36]  source map, azimuth padded circularly by 2 on both sides (column = l + 2)
#define CVA_TP 4320       // [5][20][36]  target map
#define CVA_SM 16376      // the two maps sit at the END of the buffer: the six-row chunk of the Winograd layer 1 takes its start
#define CVA_TB 18536      //   (18536 + 3 * 18 * 36 = 20480 = CV_BUF)
#define CVA_XC 0          // [96 = (k', c)][CW_CSX]: six layer-0 rows n' of 18 columns in rows of CW_RSX, channel-major
#define CW_RSX 18         // (rows of 24 and channels 160 apart -- the two tile rows of an M-tile and the two channels of a half-wave on
#define CW_CSX 112        //   the four quarters of the 64 banks, conflict-free -- measured +-0 against this compact layout)
#define CVA_XCH (96 * CW_CSX)      // 2 x 8 x 64 float4 of partial sums handed over per chunk
static_assert(CVA_XCH + 2 * 8 * 64 * 4 <= CVA_SM, "the exchange slots fit between the chunk and the layer-0 maps");

// S-term: A[m=(k',j)][(dk,e), c] = S[c][k'+dk][(j+e) mod 20], e = -2..2;  K = (dk*5 + e+2)*32 + c  (30 groups of 16)
struct SLoader {
    const float* base;                                   // SP + (k'*24 + j)*36 + lk*4   (column j + (e+2) holds azimuth j + e)
    __device__ __forceinline__ void load(float (&a)[4][1], int g) const
    {
        const int tap = g >> 1, cg = g & 1, dk = tap / 5, e2 = tap - dk * 5;
        const cvx4 v = *reinterpret_cast<const cvx4*>(base + (dk * 24 + e2) * CV_C32 + cg * 16);
#pragma unroll
        for (int p = 0; p < 4; p++) a[p][0] = v[p];
    }
};

// T-term: A[m=(k',l')][(dk,dl), c] = T[c][k'+dk][l'+dl];  K = (dk*3 + dl)*32 + c  (18 groups)
struct TLoader {
    const float* base;                                   // TP + (k'*20 + l')*36 + lk*4
    __device__ __forceinline__ void load(float (&a)[4][1], int g) const
    {
        const int tap = g >> 1, cg = g & 1, dk = tap / 3, dl = tap - dk * 3;
        const cvx4 v = *reinterpret_cast<const cvx4*>(base + (dk * 20 + dl) * CV_C32 + cg * 16);
#pragma unroll
        for (int p = 0; p < 4; p++) a[p][0] = v[p];
    }
};

// layers 2..9: valid (KW x KW) convolution over an LDS-resident [WIN*WIN][CIN+4] map;  K = (dn*KW + dl)*CIN + c.
// The tap loop is a runtime loop, the CIN/16 channel groups of a tap are unrolled: inside a tap every LDS and
// weight offset is an immediate on one per-tile base register, so a group of 4 k-steps issues only its loads
// (one ds_read_b128 per M-tile, one global_load_dwordx4 per N-tile) and its MFMAs.
// Operands of group g+1 (possibly the first group of the next tap) are loaded while group g multiplies.
// INPLACE: `out` is the buffer `in` lives in (all four wavefronts take part): the accumulators ARE the outputs, so they simply
// wait for the barrier that ends everybody's reads -- one 75 KB buffer instead of two, i.e. two workgroups per CU (round 3).
template <int MT, int NT, int CIN, int COUT, int WIN, int KW, bool INPLACE>
__device__ __forceinline__ void cv_conv_layer(const float* in, float* out, const float* __restrict__ wt,
                                              const float* __restrict__ bias, int nt0, bool relu)
{
    constexpr int WOUT = WIN - KW + 1, P = WOUT * WOUT, GPT = CIN / 16, TAPS = KW * KW, NTOT = COUT / 16;
    constexpr int CSI = CIN + 4, CSO = COUT + 4;                        // position-row strides of the two maps
    static_assert(GPT % 2 == 0, "two pipeline slots alternate per channel group");
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));       // lane-derived addresses are formed per layer (hoisted to the kernel's start they are spilled)
    const int li = lane & 15, lk = lane >> 4;
    const float* pa[MT];                 // lane's 4 channels (4lk..4lk+3 of group 0) of tile t at tap (0,0)
#pragma unroll
    for (int t = 0; t < MT; t++) {
        int m = t * 16 + li;
        m = m < P ? m : P - 1;           // padding rows of the last tile recompute position P-1 (never stored)
        pa[t] = in + ((m / WOUT) * WIN + (m % WOUT)) * CSI + lk * 4;
    }
    const float* wl = wt + ((size_t)nt0 * 64 + lane) * 4;
    cvx4 acc[MT][NT];                    // start at the bias of the output channel (C/D layout: column = lane & 15)
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const float bv = bias[(nt0 + u) * 16 + li];
#pragma unroll
        for (int t = 0; t < MT; t++) acc[t][u] = (cvx4){ bv, bv, bv, bv };
    }
    float a[2][4][MT], b[2][4][NT];
#define CVC_LOAD(SLOT, PTRS, WTAP, CG)                                                                    \
    {                                                                                                     \
        cv_gptr wg_ = (cv_gptr)((WTAP) + (size_t)(CG) * NTOT * 256);                                      \
        asm volatile("" : "+v"(wg_));                                                                     \
        _Pragma("unroll") for (int u = 0; u < NT; u++) {                                                  \
            const cvx4 bv_ = wg_[u * 64];                                                                 \
            _Pragma("unroll") for (int p = 0; p < 4; p++) b[SLOT][p][u] = bv_[p];                         \
        }                                                                                                 \
        _Pragma("unroll") for (int t = 0; t < MT; t++) {                                                  \
            const cvx4 av_ = *reinterpret_cast<const cvx4*>(PTRS[t] + (CG) * 16);                         \
            _Pragma("unroll") for (int p = 0; p < 4; p++) a[SLOT][p][t] = av_[p];                         \
        }                                                                                                 \
    }
    const float* cur[MT];
    const float* nxt[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) cur[t] = pa[t];
    const float* wcur = wl;
    CVC_LOAD(0, cur, wcur, 0)
#pragma unroll 1
    for (int tap = 0; tap < TAPS; tap++) {
        const int tn = tap + 1 < TAPS ? tap + 1 : tap;       // the last tap prefetches itself again (unused)
        const int offn = ((tn / KW) * WIN + (tn % KW)) * CSI;
#pragma unroll
        for (int t = 0; t < MT; t++) nxt[t] = pa[t] + offn;
        const float* wnxt = wl + (size_t)tn * GPT * NTOT * 256;
#pragma unroll
        for (int cg = 0; cg < GPT; cg++) {
            __builtin_amdgcn_sched_barrier(0);
            if (cg + 1 < GPT) CVC_LOAD((cg + 1) & 1, cur, wcur, cg + 1)
            else              CVC_LOAD((cg + 1) & 1, nxt, wnxt, 0)
    #pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int t = 0; t < MT; t++)
#pragma unroll
                    for (int u = 0; u < NT; u++)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cg & 1][p][t], b[cg & 1][p][u], acc[t][u], 0, 0, 0);
            CV_SCHED_TAIL(4 * MT * NT, MT + NT)
        }
#pragma unroll
        for (int t = 0; t < MT; t++) cur[t] = nxt[t];
        wcur = wnxt;
    }
#undef CVC_LOAD
    if constexpr (INPLACE) __syncthreads();          // every wavefront has finished reading the map this one overwrites
    // epilogue: ReLU + store; C/D layout: a lane holds channel n at the four positions m = 16t + 4lk + r
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int n = (nt0 + u) * 16 + li;
#pragma unroll
        for (int t = 0; t < MT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = t * 16 + lk * 4 + r;
                float v = acc[t][u][r];
                if (relu) v = fmaxf(v, 0.f);
                if (m < P) out[m * CSO + n] = v;
            }
    }
}

// ---- layers 2..5 in the Winograd F(2x2, 3x3) domain (round 3) -------------------------------------------------------------
// The (3,1,3) layers are unpadded 3x3 correlations over the (n, l) map: 16 -> 14 -> 12 -> 10 -> 8.  With the output cut into 2 x 2
// tiles they run as the 16 component GEMMs of csrc/convnet_wg.hip (wg_round: the same passes, input transform, weight ring and
// filter tiling) over M-tiles of whole tile rows -- 64 / 48 / 32 / 16 tile rows instead of 13 / 9 / 7 / 4 M-tiles x 9 taps:
// 0.55 / 0.59 / 0.51 / 0.44 of the direct form's matrix instructions, 69 % of the kernel's before.  These maps are
// CHANNEL-major, [C][CS] with rows of RS floats (a window row of a tile = two ds_read_b64); CS is chosen per map so that the two
// channels a half-wave reads land on different banks.  A wavefront owns an N-tile pair where the layer has 8 N-tiles or can
// split its M-tiles evenly (one transform feeds 8 MFMAs), and holds its outputs in registers until every wavefront has read.
template <int HIN, int TYPM>
__device__ __forceinline__ bool cw_tile(int t, int li, int& ty, int& tx)
{
    constexpr int NTY = (HIN - 2) / 2;                   // tiles per row and per column
    const int q = li / NTY;
    ty = t * TYPM + q; tx = li - q * NTY;
    return q < TYPM && ty < NTY;
}

// outputs of one M-tile of one N-tile: ReLU, then into the channel-major map [C][CSO] (rows of RSO) or, for the layer that
// feeds the direct-form layers again, position-major [(row, col)][CSO]
template <int HIN, int TYPM, int RSO, int CSO, bool POSMAJOR>
__device__ __forceinline__ void cw_store_tile(const wgf4 (&Yt)[2][2], int t, int nt, float* __restrict__ out, int li, int lk)
{
    int ty, tx;
    if (!cw_tile<HIN, TYPM>(t, li, ty, tx)) return;
    const int n0 = nt * 16 + lk * 4;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int row = 2 * ty + u, col = 2 * tx;
        if constexpr (POSMAJOR) {
#pragma unroll
            for (int v = 0; v < 2; v++) {
                wgf4 y;
#pragma unroll
                for (int r = 0; r < 4; r++) y[r] = fmaxf(Yt[u][v][r], 0.f);
                *reinterpret_cast<wgf4*>(out + (row * (HIN - 2) + col + v) * CSO + n0) = y;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                *reinterpret_cast<wgf2*>(out + (n0 + r) * CSO + row * RSO + col) = (wgf2){ fmaxf(Yt[u][0][r], 0.f), fmaxf(Yt[u][1][r], 0.f) };
        }
    }
}

// One Winograd layer over the map in `map` (HIN x HIN, rows of RS, channel stride CS), rewritten in place: this wavefront's
// N-group `ng` (NN N-tiles) over the M-tiles t0 .. t0 + MT - 1 in one round and MT2 more in a second one.
template <int HIN, int RS, int CS, int TYPM, int CIN, int NN, int MT, int MT2, int RSO, int CSO, bool POSMAJOR>
__device__ __forceinline__ void cw_layer(float* __restrict__ map, const float* __restrict__ wt, const float* __restrict__ bias, int ng, int t0)
{
    static_assert(MT >= 1 && MT <= 2 && MT2 >= 0 && MT2 <= 1 && RS % 2 == 0 && CS % 2 == 0, "");
    constexpr unsigned KSTEP = 16u * CS;
    constexpr int k4 = CIN / 4, wstride = 256 * NN;
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));
    const int li = lane & 15, lk = lane >> 4;
    const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)map;
    auto rows = [&](int t, unsigned (&ra)[4]) __attribute__((always_inline)) {
        int ty, tx;
        if (!cw_tile<HIN, TYPM>(t, li, ty, tx)) { ty = 0; tx = 0; }              // idle lanes recompute tile (0, 0), never stored
#pragma unroll
        for (int a = 0; a < 4; a++) ra[a] = base + 4u * (unsigned)(lk * CS + (2 * ty + a) * RS + 2 * tx);
    };
    unsigned RA[3][4];
    rows(t0, RA[0]);
    rows(t0 + (MT > 1 ? 1 : 0), RA[1]);
    rows(t0, RA[2]);
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned wp = (unsigned)ng * (CIN * NN * 256);          // [N-group][i 0..3][k-step][n2][lane][j]
    const unsigned lofs = lane * 16;
    const float* bl = bias + ng * NN * 16 + lk * 4;
    wgf4 W[NN][2];
    wg_first_weights<NN, 0, 2>(rs, wp, lofs, wstride, W);
    wgf4 Y[NN][3][2][2];
    wg_round<NN, 0, MT, KSTEP, true>(RA, rs, wp, wp, lofs, k4 >> 2, wstride, (unsigned)(k4 * wstride), bl, W, Y);
    wgf4 Y2[NN][3][2][2];
    if constexpr (MT2 > 0) {
        rows(t0 + MT, RA[0]);
        wg_round<NN, 0, 1, KSTEP, true>(RA, rs, wp, wp, lofs, k4 >> 2, wstride, (unsigned)(k4 * wstride), bl, W, Y2);
    }
    __syncthreads();                         // every wavefront has finished reading the map
#pragma unroll
    for (int n = 0; n < NN; n++) {
#pragma unroll
        for (int t = 0; t < MT; t++) cw_store_tile<HIN, TYPM, RSO, CSO, POSMAJOR>(Y[n][t], t0 + t, ng * NN + n, map, li, lk);
        if constexpr (MT2 > 0) cw_store_tile<HIN, TYPM, RSO, CSO, POSMAJOR>(Y2[n][0], t0 + MT, ng * NN + n, map, li, lk);
    }
}
#define CW_CS1 272        // channel strides of the maps after layers 1, 2 (= 16 mod 64: the two tile rows of an M-tile leave the
#define CW_CS2 208        //   banks 16..31 / 48..63 to the half-wave's second channel), 3 and 4 (= 32 mod 64)
#define CW_CS3 160
#define CW_CS5 72         // channel stride of layer 5's channel-major 8 x 8 map in front of a Winograd layer 6 (= 8 mod 64: the three tile rows of
                          //   layer 6's M-tile start on the banks 0, 16, 32 and take six each; the half-wave's second channel takes the six from 8, 24, 40 on)

// six layer-0 rows n' = r0 .. r0+5 into the channel-major chunk: X[(k', o)][t * 18 + l'] = relu(Smap[k'][(l'-n') mod 20][o] + Tb[k'][l'][o])
__device__ __forceinline__ void form_rows_cm(float* __restrict__ X, const float* __restrict__ SM, const float* __restrict__ TB, int r0)
{
    for (int i = threadIdx.x; i < 6 * 54 * 8; i += CV_THREADS) {
        const int c4 = i & 7, rem = i >> 3, t = rem / 54, pos = rem - t * 54;
        const int kq = pos / 18, lq = pos - kq * 18;
        int j = lq - (r0 + t);
        j = j < 0 ? j + 20 : j;
        const cvx4 sv = *reinterpret_cast<const cvx4*>(SM + (kq * 20 + j) * CV_C32 + c4 * 4);
        const cvx4 tv = *reinterpret_cast<const cvx4*>(TB + pos * CV_C32 + c4 * 4);
        float* d = X + (kq * 32 + c4 * 4) * CW_CSX + t * CW_RSX + lq;
#pragma unroll
        for (int q = 0; q < 4; q++) d[q * CW_CSX] = fmaxf(sv[q] + tv[q], 0.f);
    }
}

// N-tiles per group in the Winograd filter tiling of layer l (1..5, the N-tiles a wavefront owns there; 0: not a Winograd layer): what
// buf_winograd_tile_filters is to be called with
extern "C" int buf_cost_winograd_group(int layer)
{
    static const int group[6] = { 0, 2, 2, 2, 2, 1 };
    return layer >= 0 && layer <= 5 ? group[layer] : 0;
}
