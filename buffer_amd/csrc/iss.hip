// N11  ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; open3d compute_iss_keypoints restated from the published form, parity
// unpinned: the contract is in include/buffer_hip.h) on the sorted radius rows of buf_grid_query.
//
//   k_iss_saliency  one wavefront per point (4 per workgroup).  The row is walked twice in trips of 64 columns.  Trip of the first walk:
//                   every lane gathers the fp32 coordinates of its column's neighbour, promotes them and puts them into LDS, the valid ones
//                   compacted in column order; lanes 0..2 then add one coordinate each, entry after entry: the mean's fixed order.  Trip
//                   of the second walk: every lane forms the six products (p_a - mu_a)(p_b - mu_b) of its neighbour into LDS, lanes 0..5
//                   add one covariance entry each in the same order.  All lanes then run the same cyclic Jacobi on the six entries (wave
//                   uniform, no divergence), lane 0 writes the eigenvalues and the saliency.
//   k_iss_nms       one wavefront per point, lanes over the columns of the non-max row: counts its entries and looks for a larger saliency.
// No float atomics and a fixed order in every sum: a point's outputs are the same bits alone, in any batch and across runs.
#include "common.h"

#define ISS_WAVES 4
#define ISS_JACOBI_SWEEPS 12

// Eigenvalues of the symmetric 3x3 matrix (a00, a01, a02, a11, a12, a22), descending: cyclic Jacobi (pivots (0,1), (0,2), (1,2)) with
// the rotation of Rutishauser (t = the smaller root, |t| <= 1), until the off-diagonal part is below 1e-20 of the diagonal's or
// ISS_JACOBI_SWEEPS sweeps are done.  A function of the six entries alone.  A zero pivot is skipped.
__device__ __forceinline__ void iss_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      // theta^2 = inf gives t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
}

__device__ __forceinline__ void iss_eigenvalues(const double C[6], double ev[3])
{
    double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
    for (int sweep = 0; sweep < ISS_JACOBI_SWEEPS; sweep++) {
        const double off = (fabs(a01) + fabs(a02)) + fabs(a12), diag = (fabs(a00) + fabs(a11)) + fabs(a22);
        if (!(off > 1e-20 * diag)) break;
        iss_jacobi_rotate(a00, a11, a01, a02, a12);               // (0,1): the third index is 2
        iss_jacobi_rotate(a00, a22, a02, a01, a12);               // (0,2): the third index is 1
        iss_jacobi_rotate(a11, a22, a12, a01, a02);               // (1,2): the third index is 0
    }
    double l1 = a00, l2 = a11, l3 = a22, t;
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    if (l2 < l3) { t = l2; l2 = l3; l3 = t; }
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    ev[0] = l1; ev[1] = l2; ev[2] = l3;
}

__global__ void __launch_bounds__(ISS_WAVES * WAVE) k_iss_saliency(const float* __restrict__ pts, int n, const int* __restrict__ nbr,
                                                                  int k_nbr, int kmax, double g21, double g32, int min_nb,
                                                                  double* __restrict__ sal, double* __restrict__ eig)
{
    __shared__ double buf[ISS_WAVES][6][WAVE];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const long long pi = (long long)blockIdx.x * ISS_WAVES + wave;
    if (pi >= n) return;                                         // wave-uniform; the waves of a workgroup share no barrier
    const size_t i = (size_t)pi;
    const int* row = nbr + i * (size_t)k_nbr;
    double (*b)[WAVE] = buf[wave];
    int m = 0;
    double acc = 0.0;                                            // lanes 0..2: the sum of one coordinate
    for (int c0 = 0; c0 < kmax; c0 += WAVE) {
        const int c = c0 + lane;
        const int j = c < kmax ? row[c] : n;
        const bool valid = (unsigned int)j < (unsigned int)n;
        const unsigned long long has = __ballot(valid);
        const int cnt = __popcll(has);
        if (valid) {
            const int slot = __popcll(has & ((1ull << lane) - 1ull));
            b[0][slot] = (double)pts[3 * (size_t)j];
            b[1][slot] = (double)pts[3 * (size_t)j + 1];
            b[2][slot] = (double)pts[3 * (size_t)j + 2];
        }
        wave_sync();
        if (lane < 3)
            for (int e = 0; e < cnt; e++) acc += b[lane][e];
        wave_sync();
        m += cnt;
    }
    double ev[3] = { 0.0, 0.0, 0.0 }, s = 0.0;
    if (m >= min_nb) {                                           // wave-uniform (min_nb >= 1: m >= 1)
        const double dm = (double)m;
        const double mu0 = __shfl(acc, 0) / dm, mu1 = __shfl(acc, 1) / dm, mu2 = __shfl(acc, 2) / dm;
        acc = 0.0;                                               // lanes 0..5: the sum of one covariance entry
        for (int c0 = 0; c0 < kmax; c0 += WAVE) {
            const int c = c0 + lane;
            const int j = c < kmax ? row[c] : n;
            const bool valid = (unsigned int)j < (unsigned int)n;
            const unsigned long long has = __ballot(valid);
            const int cnt = __popcll(has);
            if (valid) {
                const int slot = __popcll(has & ((1ull << lane) - 1ull));
                const double d0 = (double)pts[3 * (size_t)j] - mu0, d1 = (double)pts[3 * (size_t)j + 1] - mu1,
                             d2 = (double)pts[3 * (size_t)j + 2] - mu2;
                b[0][slot] = d0 * d0; b[1][slot] = d0 * d1; b[2][slot] = d0 * d2;
                b[3][slot] = d1 * d1; b[4][slot] = d1 * d2; b[5][slot] = d2 * d2;
            }
            wave_sync();
            if (lane < 6)
                for (int e = 0; e < cnt; e++) acc += b[lane][e];
            wave_sync();
        }
        double C[6];
        for (int e = 0; e < 6; e++) C[e] = __shfl(acc, e) / dm;
        iss_eigenvalues(C, ev);
        if (ev[0] > 0.0 && ev[1] < g21 * ev[0] && ev[2] < g32 * ev[1]) s = ev[2];
    }
    if (lane == 0) {
        sal[i] = s;
        if (eig) { eig[3 * i] = ev[0]; eig[3 * i + 1] = ev[1]; eig[3 * i + 2] = ev[2]; }
    }
}

__global__ void __launch_bounds__(ISS_WAVES * WAVE) k_iss_nms(int n, const int* __restrict__ nbr, int k_nbr, int kmax, int min_nb,
                                                             const double* __restrict__ sal, unsigned char* __restrict__ mask)
{
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const long long pi = (long long)blockIdx.x * ISS_WAVES + wave;
    if (pi >= n) return;
    const size_t i = (size_t)pi;
    const double si = sal[i];
    unsigned char keep = 0;
    if (si > 0.0) {                                              // wave-uniform
        const int* row = nbr + i * (size_t)k_nbr;
        int m = 0;
        bool beaten = false;
        for (int c0 = 0; c0 < kmax; c0 += WAVE) {
            const int c = c0 + lane;
            const int j = c < kmax ? row[c] : n;
            const bool valid = (unsigned int)j < (unsigned int)n;
            m += __popcll(__ballot(valid));
            if (valid && sal[j] > si) beaten = true;
        }
        keep = (m >= min_nb && __ballot(beaten) == 0ull) ? 1 : 0;
    }
    if (lane == 0) mask[i] = keep;
}

extern "C" int buf_iss_keypoints(const float* pts, int n, const int* nbr_sal, int k_sal, const int* nbr_nms, int k_nms, int max_nn,
                                 double gamma_21, double gamma_32, int min_neighbors, double* saliency_out, double* eig_out,
                                 unsigned char* mask_out, void* stream)
{
    BUF_REQUIRE(n >= 0, BUF_EINVAL, "buf_iss_keypoints: n=%d", n);
    BUF_REQUIRE(k_sal >= 1, BUF_EINVAL, "buf_iss_keypoints: k_sal=%d", k_sal);
    BUF_REQUIRE(k_nms >= 1, BUF_EINVAL, "buf_iss_keypoints: k_nms=%d", k_nms);
    BUF_REQUIRE(max_nn >= 0, BUF_EINVAL, "buf_iss_keypoints: max_nn=%d", max_nn);
    BUF_REQUIRE(min_neighbors >= 1, BUF_EINVAL, "buf_iss_keypoints: min_neighbors=%d", min_neighbors);
    BUF_REQUIRE(gamma_21 > 0.0 && gamma_21 < __builtin_inf(), BUF_EINVAL, "buf_iss_keypoints: gamma_21=%g (finite, > 0)", gamma_21);
    BUF_REQUIRE(gamma_32 > 0.0 && gamma_32 < __builtin_inf(), BUF_EINVAL, "buf_iss_keypoints: gamma_32=%g (finite, > 0)", gamma_32);
    if (n == 0) return BUF_OK;
    BUF_REQUIRE(pts, BUF_EINVAL, "buf_iss_keypoints: null input pts");
    BUF_REQUIRE(nbr_sal, BUF_EINVAL, "buf_iss_keypoints: null input nbr_sal");
    BUF_REQUIRE(nbr_nms, BUF_EINVAL, "buf_iss_keypoints: null input nbr_nms");
    BUF_REQUIRE(saliency_out, BUF_EINVAL, "buf_iss_keypoints: null output saliency_out");
    BUF_REQUIRE(mask_out, BUF_EINVAL, "buf_iss_keypoints: null output mask_out");
    hipStream_t s = (hipStream_t)stream;
    const int ks = max_nn && max_nn < k_sal ? max_nn : k_sal, kn = max_nn && max_nn < k_nms ? max_nn : k_nms;
    const int blocks = cdiv(n, ISS_WAVES);
    TimedSpan span;                                               // (measurement aid, off by default: tools/iss_time.py)
    bool timed = timing_begin(s, &span, ((4.0 * k_sal + 24.0 * ks) + 32.0) * n, BUF_TIMED_ISS_SALIENCY);
    k_iss_saliency<<<blocks, ISS_WAVES * WAVE, 0, s>>>(pts, n, nbr_sal, k_sal, ks, gamma_21, gamma_32, min_neighbors, saliency_out, eig_out);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, ((4.0 * k_nms + 8.0 * kn) + 9.0) * n, BUF_TIMED_ISS_NMS);
    k_iss_nms<<<blocks, ISS_WAVES * WAVE, 0, s>>>(n, nbr_nms, k_nms, kn, min_neighbors, saliency_out, mask_out);
    if (timed) timing_end(s, &span);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
