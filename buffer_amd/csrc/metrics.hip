// Per-stage ground-truth metrics of B registered pairs (keypoint repeatability, inlier counts of the putative and the mutual
// matches, the consensus set of the returned pose): a diagnostic beside the registration path, not part of it.  One launch.
//
//   k_match_metrics   one workgroup per (tile of MET_TILE query keypoints, direction, pair).  Direction 0: the queries are the
//                     pair's source keypoints under T_gt, the other cloud its target keypoints; direction 1: the target keypoints
//                     under the inverse of T_gt against the source keypoints.  The other cloud goes through LDS in tiles of
//                     MET_REF rows (every lane reads the same row: a broadcast, no bank conflict); each thread keeps the running
//                     d2 minimum of its own query, rows in ascending order with a strict <: the lowest row keeps a tie (the row
//                     itself is not an output, so only its d2 is carried) and a NaN / inf d2 never wins.  The direction-0
//                     blocks also classify their queries' matches (one gather of the matched target keypoint per thread).
//                     Counts are summed inside the wave by ballot and added to the pair's row with one integer atomicAdd per
//                     wave and column (integer sums do not depend on the order).
// Arithmetic (include/buffer_hip.h, buf_match_metrics): p = T s in fp64 without FMA, rounded to fp32; d2 by sqdist3.
#include "common.h"

#define MET_TILE 256
#define MET_REF 1024

struct MetRigid { double r[3][3], t[3]; };

// rows 0..2 of a row-major 4x4 (E = double or float, widened exactly)
template <typename E>
__device__ __forceinline__ MetRigid met_load(const E* __restrict__ T)
{
    MetRigid m;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) m.r[i][j] = (double)T[4 * i + j];
        m.t[i] = (double)T[4 * i + 3];
    }
    return m;
}

// [R^T, -R^T t]: row i of the inverse is column i of R; its translation is -((R0i*t0 + R1i*t1) + R2i*t2)
__device__ __forceinline__ MetRigid met_inverse(const MetRigid& m)
{
    MetRigid v;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) v.r[i][j] = m.r[j][i];
        v.t[i] = -((m.r[0][i] * m.t[0] + m.r[1][i] * m.t[1]) + m.r[2][i] * m.t[2]);
    }
    return v;
}

__device__ __forceinline__ void met_apply(const MetRigid& m, float x, float y, float z, float& px, float& py, float& pz)
{
    const double sx = x, sy = y, sz = z;
    px = (float)(((m.r[0][0] * sx + m.r[0][1] * sy) + m.r[0][2] * sz) + m.t[0]);
    py = (float)(((m.r[1][0] * sx + m.r[1][1] * sy) + m.r[1][2] * sz) + m.t[1]);
    pz = (float)(((m.r[2][0] * sx + m.r[2][1] * sy) + m.r[2][2] * sz) + m.t[2]);
}

// number of threads of the wave with `flag`, added to *dst by lane 0 (one atomic per wave)
__device__ __forceinline__ void met_wave_count(bool flag, int* __restrict__ dst)
{
    const int n = __popcll(__ballot(flag));
    if ((threadIdx.x & (WAVE - 1)) == 0 && n) atomicAdd(dst, n);
}

__global__ void __launch_bounds__(MET_TILE) k_match_metrics(const float* __restrict__ kp, const int* __restrict__ s_nn,
                                                          const int* __restrict__ t_nn, int P, const double* __restrict__ T_gt,
                                                          const float* __restrict__ T_est, float kp2, float match2, float cons2,
                                                          int* __restrict__ counts, float* __restrict__ nn_d2)
{
    __shared__ float4 ref[MET_REF];
    const int b = blockIdx.z, dir = blockIdx.y;
    const int q = blockIdx.x * MET_TILE + threadIdx.x;
    const bool live = q < P;
    const size_t qbase = ((size_t)2 * b + dir) * P, rbase = ((size_t)2 * b + (1 - dir)) * P;       // query cloud, other cloud
    const MetRigid gt = met_load(T_gt + 16 * (size_t)b);
    float px = 0.f, py = 0.f, pz = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    if (live) {
        sx = kp[3 * (qbase + q)]; sy = kp[3 * (qbase + q) + 1]; sz = kp[3 * (qbase + q) + 2];
        if (dir == 0) met_apply(gt, sx, sy, sz, px, py, pz);
        else met_apply(met_inverse(gt), sx, sy, sz, px, py, pz);
    }
    float best = __builtin_inff();
    for (int lo = 0; lo < P; lo += MET_REF) {
        const int n = min(MET_REF, P - lo);
        __syncthreads();                                                  // (the previous tile has been read by every wave)
        for (int i = threadIdx.x; i < n; i += MET_TILE) {
            const size_t r = 3 * (rbase + lo + i);
            ref[i] = make_float4(kp[r], kp[r + 1], kp[r + 2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < n; i++) {
            const float4 c = ref[i];
            const float d2 = sqdist3(px, py, pz, c.x, c.y, c.z);
            best = d2 < best ? d2 : best;                                 // ascending rows, strict <: the lowest row keeps a tie
        }
    }
    int* row = counts + BUF_METRICS_NCOUNT * (size_t)b;
    if (live && nn_d2) nn_d2[qbase + q] = best;
    met_wave_count(live && best < kp2, row + (dir == 0 ? BUF_METRICS_REP_SRC : BUF_METRICS_REP_TGT));
    if (dir != 0) return;                                                 // (uniform per block)

    // the matches of source keypoint q: putative = its descriptor-space 1-NN t, mutual when t's 1-NN is q
    bool nn_inl = false, mutual = false, cons = false;
    if (live) {
        const int t = s_nn[(size_t)b * P + q];
        if (t >= 0 && t < P) {                                            // (an index outside the cloud matches nothing)
            const size_t r = 3 * (rbase + t);
            const float tx = kp[r], ty = kp[r + 1], tz = kp[r + 2];
            nn_inl = sqdist3(px, py, pz, tx, ty, tz) < match2;
            mutual = t_nn[(size_t)b * P + t] == q;
            float ex, ey, ez;
            met_apply(met_load(T_est + 16 * (size_t)b), sx, sy, sz, ex, ey, ez);
            cons = mutual && sqdist3(ex, ey, ez, tx, ty, tz) < cons2;
        }
    }
    met_wave_count(nn_inl, row + BUF_METRICS_NN_INL);
    met_wave_count(mutual, row + BUF_METRICS_MUTUAL);
    met_wave_count(mutual && nn_inl, row + BUF_METRICS_MUTUAL_INL);
    met_wave_count(cons, row + BUF_METRICS_CONS);
    met_wave_count(cons && nn_inl, row + BUF_METRICS_CONS_TRUE);
}

static bool met_threshold_ok(float v) { return v > 0.f && v <= 3.4e38f; }       // (false for NaN)

extern "C" int buf_match_metrics(const float* kp, const int* s_nn, const int* t_nn, int npairs, int P, const double* T_gt_f64,
                                 const float* T_est_f32, float tau_kp, float tau_match, float dist_th, int* out_counts,
                                 float* out_nn_d2, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(npairs >= 0 && P >= 0, BUF_EINVAL, "buf_match_metrics: npairs=%d P=%d", npairs, P);
    BUF_REQUIRE(met_threshold_ok(tau_kp), BUF_EINVAL, "buf_match_metrics: tau_kp=%g (must be finite and > 0)", (double)tau_kp);
    BUF_REQUIRE(met_threshold_ok(tau_match), BUF_EINVAL, "buf_match_metrics: tau_match=%g (must be finite and > 0)", (double)tau_match);
    BUF_REQUIRE(met_threshold_ok(dist_th), BUF_EINVAL, "buf_match_metrics: dist_th=%g (must be finite and > 0)", (double)dist_th);
    if (npairs == 0 || P == 0) return BUF_OK;
    BUF_REQUIRE(kp && s_nn && t_nn && T_gt_f64 && T_est_f32 && out_counts, BUF_EINVAL, "buf_match_metrics: null argument");
    BUF_REQUIRE(npairs <= 65535, BUF_EINVAL, "buf_match_metrics: %d pairs (at most 65535 per call)", npairs);
    BUF_REQUIRE(2LL * npairs * P < 0x7fffffffLL / 3, BUF_EINVAL, "buf_match_metrics: %lld keypoints (int32 indices)", 2LL * npairs * P);
    BUF_CHECK_HIP(hipMemsetAsync(out_counts, 0, sizeof(int) * BUF_METRICS_NCOUNT * (size_t)npairs, s));
    k_match_metrics<<<dim3(cdiv(P, MET_TILE), 2, npairs), MET_TILE, 0, s>>>(kp, s_nn, t_nn, P, T_gt_f64, T_est_f32, tau_kp * tau_kp,
                                                                             tau_match * tau_match, dist_th * dist_th, out_counts,
                                                                             out_nn_d2);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
