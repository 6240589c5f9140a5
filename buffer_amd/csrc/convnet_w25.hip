// A11 dense part -- w25_layer_psplit, a layer form of the fused kernel (cyl_net_w25t_body, csrc/convnet_w25t.hip): F(2x5, 3x3) tiles in
// every layer the caller hands an F(2x5) filter set for.  Tiles of 2 rows x 5 azimuth columns carry the 7 x 20 map with exactly 4 x 4 = 16 regular tiles -- ONE full
// M-tile, row 7 of the bottom tile row dropped -- where F(2x4) needs 17.5 tiles of 8 outputs, hence its special sixteenth lane and its
// direct round of row 6, columns 0..15.  4 row components x 7 column components = 28 matrix instructions per (k-step, N-tile) against
// 24 + 6; no direct round, no special lane, no row-6 store path.  Every layer without such a set runs in its F(2x4) or F(2x2) form.
//
//     Y = A2^T [ sum_c (G2 g G5^T)[c] (.) (B2^T d[c] B5) ] A5        F(2,3) down the rows as before, F(5,3) along the azimuth on the seven
//                                                                    points 0, +-1, +-2, +-1/2 (tools/f25_restate.py picked them)
//
// Tile geometry.  Lane column li holds tile (ty = li >> 2, tx = li & 3): output rows 2 ty, 2 ty + 1, output columns 5 tx .. 5 tx + 4.
// Its window: rows 2 ty - 1 .. 2 ty + 2, seven words from word 5 tx of the row layout (WG_ROW = 22 words: column 19, columns 0..19,
// column 0; the last window ends at word 21).  The window starts at an odd word for odd tx: the words are read with 4-byte-aligned
// instructions (ds_read2_b32, four per row), not with the three ds_read_b64 of W24_LOAD.
//
// Padding rows.  The zero area of a channel (four zeros, two dump words) is one word short of a window row, so no window row is read
// from it.  The row combination of the pass split is one v_fma per word, da + fac db; here fac is per LANE and both row addresses point
// into the map:
//     db in the elevation padding (ty = 3: rows 7, 8)     db := da's row,  fac = 0         da + 0 da = da
//     da in the elevation padding (row -1, or row 7)      da := db's row,  fac = sgn - 1   db + (sgn - 1) db = sgn db  (sgn = -1 there:
//                                                                                          d - 2 d = -d, exact)
// Both are exact for finite d; a non-finite d gives NaN where a true zero row would have kept it (0 x inf) -- in the plain kernel and
// in the masked re-run alike: both run this body on the same input words in the same order, so they agree bit for bit on every patch,
// finite or not.  The padding rows read nothing, so the layer needs neither the dump-word clear nor the barrier behind it.
//
// The layer form (w25_layer_psplit<NT, GLB>): w24p_layer_psplit's pass split.  Wavefront w owns row component I = w for all NT N-tiles
// (NT = 4: 64 outputs, NT = 2: 32 outputs) over the whole K: per k-step two window rows (eight LDS reads), one transform of 28 vector
// instructions (7 row combinations, 3 for point 0, 6 per +- pair: an even part on words 2, 4, 6 and an odd part on words 1, 3, 5), 7 NT
// MFMAs into 28 NT accumulators (24 NT in accumulation registers beside the 13 parked window addresses of the other layer forms, the
// 4 NT of column component 6 in vector registers: see W25_MFMA; this form's own two addresses and its factor are formed per layer from
// the lane number and parked nowhere).  The filter ring holds two k-steps: 7 NT x 2 = 56 vector registers at NT = 4.  A5^T is folded once after the loop (f_I: NT N-tiles x 5
// columns x wgf4, 80 floats per lane at NT = 4); the bias rides in the column component of point +1 of row component 1, which A5^T
// carries into all five columns and A2^T into both rows with weight 1.  Wavefront q < NT finishes N-tile q:
//     row 0 = (f_0 + f_1) + f_2,     row 1 = (f_1 - f_2) - f_3.
//
// The exchange.  Every wavefront hands f_w of the N-tiles q != w to their finishers, 5 float4 per lane and receiver (60 floats per lane
// at NT = 4, 61 KB of the 80 KB buffer, which is free behind the barrier that says every wavefront has read the layer's input):
//   * three float4 (columns 0..2) into the RECEIVER's own output rows: channel 16 q + (lane >> 2), words 36 (lane & 3) + 12 rank + 4 v
//     (rank: the sender's place among q's three senders) -- words 0..143 of the rows 0..16 NT - 1.  Only q overwrites these rows, with
//     its own stores, after it has read them: no third barrier.
//   * two float4 (columns 3, 4) into the SENDER's rows of the wide area: channel 64 + 16 w + (lane >> 2), words 24 (lane & 3) + 8 slot
//     + 4 (v - 3) (slot: q's place among w's receivers) -- words 0..95 of the rows 64..127.
// Words WG_ZERO..WG_ZERO + 3 of every channel are not touched (a later layer in the F(2x4) form reads them as padding); the dump words
// take what the stores have no place for, as in every other form, and the forms that read them clear them first.
// Barriers per layer, beside the one that closes every layer: two (input read | exchange in place).
//
// Stores: 2 rows x 5 words per tile and channel, the halo copy of column 0 behind column 19 from tx = 0 and of column 19 in front of
// column 0 from tx = 3; the bottom tile row's second row (row 7) goes to the dump words.  The last layer stores to global memory.
#include "common.h"

#define W25_FLAG 8             // bit 3 of the kernel's relu word (set by the launcher only): P.wt[l] IS the layer's F(2x5) set
#define W25_TILE 448           // floats per (row component, k-step, N-tile): 256 (j = 0..3) + 128 (j = 4, 5) + 64 (j = 6)
#define W25_XCH_C 64           // first channel row of the wide part of the exchange area
#define W25_XCH_WIDE 24        // words per lane there (two float4 per receiver)
#define W25_XCH_OWN 36         // words per lane in a receiver's own rows (three float4 per sender)

typedef const __attribute__((address_space(3))) float* wg_lds_f1;

__device__ __forceinline__ float w25_ldw1(__amdgpu_buffer_rsrc_t rs, unsigned uniform_float_ofs, unsigned lane_byte_ofs)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, lane_byte_ofs, uniform_float_ofs * 4, 0));
}

// The accumulators of the column components 0..5 live in accumulation registers (W24P_MFMA, csrc/convnet_w24p.hip); those of component 6
// in vector registers, of which the pass leaves more than forty free: 24 NT + 13 parked addresses leave the accumulation half the room
// the other layer forms' loops need for what they carry across (with all 28 NT there the kernel spilled: profiles/f25_ab.md).
#define W25_MFMA_V(PRE, ACC, A, B) asm volatile(PRE "v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(ACC) : "v"(A), "v"(B));
#define W25_MFMA(PRE, J, ACC, A, B)                                                                       \
    {                                                                                                     \
        if ((J) < 6) W24P_MFMA(PRE, ACC, A, B)                                                            \
        else W25_MFMA_V(PRE, ACC, A, B)                                                                   \
    }

// component j = 0..6 of N-tile n's block row in ring slot k
#define W25_U(n, k, j) ((j) < 4 ? W4[n][k][j] : ((j) < 6 ? W2[n][k][(j) - 4] : W1[n][k]))

// Two window rows of seven words at 4-byte alignment (the compiler pairs them into ds_read2_b32)
#define W25_LOAD(DST, A0, A1_, OFS)                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int q_ = 0; q_ < 7; q_++) DST[q_] = *(wg_lds_f1)(size_t)((A0) + (OFS) + 4 * q_);       \
        _Pragma("unroll") for (int q_ = 0; q_ < 7; q_++) DST[7 + q_] = *(wg_lds_f1)(size_t)((A1_) + (OFS) + 4 * q_);  \
    }

// Row component da + fac db of the seven window words in D (one v_fma per word), then B5^T, rows scaled to dyadic coefficients:
//     t0   = (r6 - r0) + 5.25 (r2 - r4)                                                   point 0:     (x^2 - 1)(x^2 - 4)(x^2 - 1/4)
//     t1,2 = (r2 - 4.25 r4 + r6) +- (r1 - 4.25 r3 + r5)                                   points +-1:  (x +- 1) x (x^2 - 4)(x^2 - 1/4)
//     t3,4 = (r2 / 4 - 1.25 r4 + r6) +- 2 (r1 / 4 - 1.25 r3 + r5)                         points +-2:  (x +- 2) x (x^2 - 1)(x^2 - 1/4)
//     t5,6 = (4 r2 - 5 r4 + r6) +- (4 r1 - 5 r3 + r5) / 2                                 points +-1/2: (x +- 1/2) x (x^2 - 1)(x^2 - 4)
// into V[BUF]; uses the caller's D, V and fac.  28 instructions.
#define W25_XFORM(BUF)                                                                                    \
    {                                                                                                     \
        float r_[7];                                                                                      \
        _Pragma("unroll") for (int b = 0; b < 7; b++) r_[b] = __builtin_fmaf(fac, D[7 + b], D[b]);        \
        V[BUF][0] = __builtin_fmaf(5.25f, wg_sub(r_[2], r_[4]), wg_sub(r_[6], r_[0]));                    \
        const float e1_ = wg_add(__builtin_fmaf(-4.25f, r_[4], r_[2]), r_[6]);                            \
        const float o1_ = wg_add(__builtin_fmaf(-4.25f, r_[3], r_[1]), r_[5]);                            \
        V[BUF][1] = wg_add(e1_, o1_); V[BUF][2] = wg_sub(e1_, o1_);                                       \
        const float e2_ = __builtin_fmaf(0.25f, r_[2], __builtin_fmaf(-1.25f, r_[4], r_[6]));             \
        const float o2_ = __builtin_fmaf(0.25f, r_[1], __builtin_fmaf(-1.25f, r_[3], r_[5]));             \
        V[BUF][3] = __builtin_fmaf(2.f, o2_, e2_); V[BUF][4] = __builtin_fmaf(-2.f, o2_, e2_);            \
        const float e3_ = __builtin_fmaf(4.f, r_[2], __builtin_fmaf(-5.f, r_[4], r_[6]));                 \
        const float o3_ = __builtin_fmaf(4.f, r_[1], __builtin_fmaf(-5.f, r_[3], r_[5]));                 \
        V[BUF][5] = __builtin_fmaf(0.5f, o3_, e3_); V[BUF][6] = __builtin_fmaf(-0.5f, o3_, e3_);          \
    }

// One k-step of the NT N-tiles' filters into ring slot `slot`: block at float offset o, N-tiles W25_TILE apart
template <int NT>
__device__ __forceinline__ void w25_ring(__amdgpu_buffer_rsrc_t rs, unsigned o, unsigned lofs4, unsigned lofs2, unsigned lofs1, int slot,
                                         wgf4 (&W4)[NT][2], wgf2 (&W2)[NT][2], float (&W1)[NT][2])
{
#pragma unroll
    for (int n = 0; n < NT; n++) {
        W4[n][slot] = wg_ldw(rs, o + n * W25_TILE, lofs4);
        W2[n][slot] = w24_ldw2(rs, o + n * W25_TILE + 256, lofs2);
        W1[n][slot] = w25_ldw1(rs, o + n * W25_TILE + 384, lofs1);
    }
}

// Row component I = w over `niter` x 4 k-steps for NT N-tiles: acc[n][j] += V_Ij(tile, c) * U_Ij(c, n).  w24p_pass's steps and fences
// (the LDS reads ONE step ahead, the filter ring two) with seven column components; P0 / P1: the two window rows (da, db), fac: the
// lane's factor of db.  On entry W holds the
// first two k-steps of the block at wp (k-steps `kstride` floats apart); the last iteration fetches the k-steps 0, 1 again (unused, in
// bounds).
template <int NT>
__device__ __forceinline__ void w25_pass(unsigned P0, unsigned P1, float fac, __amdgpu_buffer_rsrc_t rs, unsigned wp, unsigned kstride, unsigned lofs4,
                                         unsigned lofs2, unsigned lofs1, int niter, wgf4 (&W4)[NT][2], wgf2 (&W2)[NT][2], float (&W1)[NT][2],
                                         wgf4 (&acc)[NT][7])
{
    float D[14];                                     // one k-step of window words in flight
    float V[2][7];
    W25_LOAD(D, P0, P1, 0)
    W25_XFORM(0)
    int it = 0;
#pragma unroll 1
    do {                                             // (niter >= 1, as in w24p_pass)
        const bool more = it + 1 < niter;
        const unsigned wcur = wp + 4 * it * kstride;                               // this iteration's k-steps 2, 3 ...
        const unsigned wn = more ? wcur + 4 * kstride : wp;                        // ... and the k-steps 0, 1 of the next one
        const unsigned adv = more ? 4u * WG_KSTEP : 0u;           // past the end: the iteration's own first steps again (unused)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (s < 3) W25_LOAD(D, P0, P1, (s + 1) * WG_KSTEP)
            else {
                P0 += adv; P1 += adv;                              // the next iteration's base
                W25_LOAD(D, P0, P1, 0)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int j = 0; j < 7; j++) {
                    if (n == 0 && j == 0) W25_MFMA("s_nop 1\n\t", j, acc[n][j], W25_U(n, s & 1, j), V[s & 1][j])
                    else W25_MFMA("", j, acc[n][j], W25_U(n, s & 1, j), V[s & 1][j])
                }
            __builtin_amdgcn_sched_barrier(0);
            W25_XFORM((s + 1) & 1)
            // k-step s is through: its registers take the k-step two further on
            w25_ring<NT>(rs, s < 2 ? wcur + (s + 2) * kstride : wn + (s - 2) * kstride, lofs4, lofs2, lofs1, s & 1, W4, W2, W1);
            __builtin_amdgcn_sched_barrier(0);
        }
    } while (++it < niter);
    // The last matrix instructions' results before anything reads them (see w24p_pass): every accumulator is an operand
#pragma unroll
    for (int n = 0; n < NT; n += 2)
        asm volatile("s_nop 15"
                     : "+a"(acc[n][0]), "+a"(acc[n][1]), "+a"(acc[n][2]), "+a"(acc[n][3]), "+a"(acc[n][4]), "+a"(acc[n][5]), "+v"(acc[n][6]),
                       "+a"(acc[n + 1][0]), "+a"(acc[n + 1][1]), "+a"(acc[n + 1][2]), "+a"(acc[n + 1][3]), "+a"(acc[n + 1][4]), "+a"(acc[n + 1][5]),
                       "+v"(acc[n + 1][6]));
}

// Wavefront W hands f_W of the N-tiles q != W (q < NT) to their finishers: three float4 to q's own rows, two to W's rows of the wide area
template <int W, int NT>
__device__ __forceinline__ void w25_give(const wgf4 (&f)[NT][5], float* __restrict__ act, int lane)
{
    float* wide = act + (W25_XCH_C + 16 * W + (lane >> 2)) * WG_CS + (lane & 3) * W25_XCH_WIDE;
#pragma unroll
    for (int q = 0; q < NT; q++) {
        if (q == W) continue;
        const int slot = q - (q > W), rank = W - (W > q);         // q among W's receivers, W among q's senders
        float* own = act + (16 * q + (lane >> 2)) * WG_CS + (lane & 3) * W25_XCH_OWN + 12 * rank;
#pragma unroll
        for (int v = 0; v < 3; v++) *reinterpret_cast<wgf4*>(own + 4 * v) = f[q][v];
#pragma unroll
        for (int v = 3; v < 5; v++) *reinterpret_cast<wgf4*>(wide + 8 * slot + 4 * (v - 3)) = f[q][v];
    }
}

// Wavefront Q < NT finishes N-tile Q: its own f_Q and the three received ones, rows combined in one order for every Q
template <int Q, int NT>
__device__ __forceinline__ void w25_take(const wgf4 (&f)[NT][5], const float* __restrict__ act, int lane, wgf4 (&Yk)[2][5])
{
#pragma unroll
    for (int v = 0; v < 5; v++) {
        wgf4 F[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int slot = Q - (Q > i), rank = i - (i > Q);
            if (i == Q) F[i] = f[Q][v];
            else if (v < 3) F[i] = *reinterpret_cast<const wgf4*>(act + (16 * Q + (lane >> 2)) * WG_CS + (lane & 3) * W25_XCH_OWN + 12 * rank + 4 * v);
            else F[i] = *reinterpret_cast<const wgf4*>(act + (W25_XCH_C + 16 * i + (lane >> 2)) * WG_CS + (lane & 3) * W25_XCH_WIDE + 8 * slot + 4 * (v - 3));
        }
        Yk[0][v] = (F[0] + F[1]) + F[2];
        Yk[1][v] = (F[1] - F[2]) - F[3];
        if (v & 1) __builtin_amdgcn_sched_barrier(0);             // (two columns at a time, as in w24p_take)
    }
}

// ReLU + store of one finished N-tile's 2 x 5 tiles: into the activation buffer with the circular halo copies (what a lane has no place
// for -- row 7, the halo copies of the inner tiles -- goes to the channel's dump words), or, for the last layer, to y[32][140]
template <bool GLB>
__device__ __forceinline__ void w25_store(const wgf4 (&Yt)[2][5], int nt, int relu, float* __restrict__ act, float* __restrict__ out_glb, int li, int lk)
{
    const int n0 = nt * 16 + lk * 4;
    const float lo = relu ? 0.f : -__builtin_inff();
    const int ty = li >> 2, tx = li & 3;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int row = 2 * ty + u;
        const bool ok = row < 7;
        if constexpr (GLB) {
            if (ok) {
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int v = 0; v < 5; v++) out_glb[(size_t)(n0 + r) * 140 + row * 20 + 5 * tx + v] = fmaxf(Yt[u][v][r], lo);
            }
        } else {
            const int pos = ok ? row * WG_ROW + 5 * tx + 1 : WG_ZERO + 4;
            const int step = ok ? 1 : 0;
            const int h0 = (ok && tx == 0) ? row * WG_ROW + 21 : WG_ZERO + 4;      // column 0 again behind column 19
            const int h1 = (ok && tx == 3) ? row * WG_ROW : WG_ZERO + 5;           // column 19 again in front of column 0
            float* p = act + n0 * WG_CS;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float val[5];
#pragma unroll
                for (int v = 0; v < 5; v++) { val[v] = fmaxf(Yt[u][v][r], lo); p[r * WG_CS + pos + v * step] = val[v]; }
                p[r * WG_CS + h0] = val[0]; p[r * WG_CS + h1] = val[4];
            }
        }
    }
}

// One layer with 16 NT output channels on F(2x5) tiles in the pass-split form; wt: the layer's F(2x5) set ([i][k-step][N-tile][448]).
// Cin % 16 == 0.  See the head of the file for the padding factor, the exchange and the barriers.
template <int NT, bool GLB>
__device__ __forceinline__ void w25_layer_psplit(float* __restrict__ act, float* __restrict__ out_glb, const float* __restrict__ wt,
                                                 const float* __restrict__ bias, int cin, int relu, int w)
{
    int lane = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane));                   // (the addresses below are formed per layer, not kept through the others)
    const int lk = lane >> 4, li = lane & 15;
    const int k4 = cin >> 2;
    const __amdgpu_buffer_rsrc_t rs = wg_weights(wt);
    const unsigned kstride = NT * W25_TILE;
    const unsigned wp = (unsigned)(w * k4) * kstride;                              // [i = w][k-step][N-tile][448]
    const unsigned lofs4 = lane * 16, lofs2 = lane * 8, lofs1 = lane * 4;
    // window rows (da, db) of row component w: (0, 2) (1, 2) (2, 1) (1, 3), db enters with sgn; a row in the elevation padding is
    // replaced by the other row and a factor (head of the file)
    const int r0 = 2 * (li >> 2) - 1;
    int rowa = r0 + (w == 0 ? 0 : (w == 2 ? 2 : 1)), rowb = r0 + (w == 3 ? 3 : (w == 2 ? 1 : 2));
    const float sgn = w == 1 ? 1.f : -1.f;
    float fac = sgn;
    if (rowb > 6) { rowb = rowa; fac = 0.f; }
    if (rowa < 0 || rowa > 6) { rowa = rowb; fac = sgn - 1.f; }
    const unsigned act_addr = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)act;
    const unsigned tile = (unsigned)(lk * WG_CS + 5 * (li & 3));
    unsigned P0 = act_addr + 4u * (tile + (unsigned)rowa * WG_ROW), P1 = act_addr + 4u * (tile + (unsigned)rowb * WG_ROW);
    wgf4 f[NT][5];                                   // f_w: [N-tile][column] after A5^T
    {
        wgf4 acc[NT][7];
        float zero = 0.f;
        asm volatile("" : "+v"(zero));               // (an opaque zero: see wg_round)
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int j = 0; j < 7; j++) acc[n][j] = (wgf4){ zero, zero, zero, zero };
        if (w == 1) {                                // the bias: once, in the column component of point +1 of row component 1
#pragma unroll
            for (int n = 0; n < NT; n++) acc[n][1] = *reinterpret_cast<const wgf4*>(bias + n * 16 + lk * 4);
        }
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int j = 0; j < 7; j++) {
                if (j < 6) asm volatile("" : "+a"(acc[n][j]));
                else asm volatile("" : "+v"(acc[n][j]));
            }
        __builtin_amdgcn_sched_barrier(0);           // (the accumulators' start first, as in w24p_layer_psplit)
        wgf4 W4[NT][2];
        wgf2 W2[NT][2];
        float W1[NT][2];
        w25_ring<NT>(rs, wp, lofs4, lofs2, lofs1, 0, W4, W2, W1);
        w25_ring<NT>(rs, wp + kstride, lofs4, lofs2, lofs1, 1, W4, W2, W1);
        w25_pass<NT>(P0, P1, fac, rs, wp, kstride, lofs4, lofs2, lofs1, k4 >> 2, W4, W2, W1, acc);
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int r = 0; r < 4; r++) {            // A5^T: row i = the i-th powers of 0, +-1, +-2, +-1/2, on shared sums and differences
                const float p1 = acc[n][1][r] + acc[n][2][r], q1 = acc[n][1][r] - acc[n][2][r];
                const float p2 = acc[n][3][r] + acc[n][4][r], q2 = acc[n][3][r] - acc[n][4][r];
                const float p3 = acc[n][5][r] + acc[n][6][r], q3 = acc[n][5][r] - acc[n][6][r];
                f[n][0][r] = (acc[n][0][r] + p1) + (p2 + p3);
                f[n][1][r] = __builtin_fmaf(2.f, q2, __builtin_fmaf(0.5f, q3, q1));
                f[n][2][r] = __builtin_fmaf(4.f, p2, __builtin_fmaf(0.25f, p3, p1));
                f[n][3][r] = __builtin_fmaf(8.f, q2, __builtin_fmaf(0.125f, q3, q1));
                f[n][4][r] = __builtin_fmaf(16.f, p2, __builtin_fmaf(0.0625f, p3, p1));
            }
    }
    __syncthreads();                                 // every wavefront has finished reading the layer's input: the whole buffer is free
    int lane_s = threadIdx.x & (WAVE - 1);
    asm volatile("" : "+v"(lane_s));                 // the exchange and store offsets are formed here, not kept from the layer's start
    if (w == 0) w25_give<0, NT>(f, act, lane_s);
    else if (w == 1) w25_give<1, NT>(f, act, lane_s);
    else if (w == 2) w25_give<2, NT>(f, act, lane_s);
    else w25_give<3, NT>(f, act, lane_s);
    __syncthreads();                                 // the exchange is in place
    if (w < NT) {
        wgf4 Yk[2][5];
        if (w == 0) w25_take<0, NT>(f, act, lane_s, Yk);
        else if (w == 1) w25_take<1, NT>(f, act, lane_s, Yk);
        else if constexpr (NT == 4) {
            if (w == 2) w25_take<2, NT>(f, act, lane_s, Yk);
            else w25_take<3, NT>(f, act, lane_s, Yk);
        }
        w25_store<GLB>(Yk, w, relu, act, out_glb, lane_s & 15, lane_s >> 4);
    }
}

// Host helper: filters w [Cout][Cin][3][3] (BN folded) -> U = G2 g G5^T in fp64, rounded once: 4 row x 7 column components (the points
// 0, +-1, +-2, +-1/2 in this order) in the tiling w25_layer_psplit streams,
//     out[28 * Cout * Cin] = [i][k-step][N-tile][ [lk][li][j = 0..3] | [lk][li][j = 4, 5] | [lk][li][j = 6] ]
// (256 + 128 + 64 floats: a lane's seven components of a block row are a 16-, an 8- and a 4-byte buffer load) of
// U[i][j][16 n + li][4 ks + lk].  No device work.
extern "C" int buf_winograd_f25_tile_weights(const float* w_host, int cout, int cin, float* out_host)
{
    BUF_REQUIRE(w_host && out_host, BUF_EINVAL, "buf_winograd_f25_tile_weights: null argument");
    BUF_REQUIRE(cout > 0 && cin > 0 && cout % 16 == 0 && cin % 4 == 0, BUF_EINVAL, "buf_winograd_f25_tile_weights: widths %d -> %d", cin, cout);
    static const double G2[4][3] = { { 1, 0, 0 }, { .5, .5, .5 }, { .5, -.5, .5 }, { 0, 0, 1 } };
    static const double pts[7] = { 0, 1, -1, 2, -2, .5, -.5 };
    double G5[7][3];
    for (int j = 0; j < 7; j++) {
        double nj = 1;                               // L_j(p_j) = prod_{k != j} (p_j - p_k)
        for (int k = 0; k < 7; k++)
            if (k != j) nj *= pts[j] - pts[k];
        G5[j][0] = 1 / nj; G5[j][1] = pts[j] / nj; G5[j][2] = pts[j] * pts[j] / nj;
    }
    const int k4 = cin / 4, ntile = cout / 16;
    for (int o = 0; o < cout; o++)
        for (int c = 0; c < cin; c++) {
            const float* g = w_host + ((size_t)o * cin + c) * 9;
            const int lane = (c % 4) * 16 + o % 16;
            for (int i = 0; i < 4; i++) {
                float* blk = out_host + (((size_t)i * k4 + c / 4) * ntile + o / 16) * W25_TILE;
                for (int j = 0; j < 7; j++) {
                    double u = 0;
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) u += G2[i][a] * (double)g[3 * a + b] * G5[j][b];
                    if (j < 4) blk[lane * 4 + j] = (float)u;
                    else if (j < 6) blk[256 + lane * 2 + (j - 4)] = (float)u;
                    else blk[384 + lane] = (float)u;
                }
            }
        }
    return BUF_OK;
}
