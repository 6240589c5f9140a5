// N6  FPFH descriptors (Rusu, Blodow, Beetz 2009; open3d compute_fpfh_feature restated, unpinned: the contract is in
// include/buffer_hip.h) on the sorted radius rows of buf_grid_query.
//
//   k_spfh   one wavefront per point (4 per workgroup), lanes over the row's columns (two trips for rows longer than 64).  A lane
//            forms the fp64 pair feature of its neighbour and adds 1 to three of the point's 33 integer counters in LDS (integer
//            LDS adds: exact and order-free); the counters are scaled once, by 100 / (m - 1), when the row is done.
//   k_fpfh   one wavefront per point.  The lanes first form the weights 1 / d2 of the row's columns (one each) and compact the
//            neighbours that carry one into LDS, in column order; lane s < 33 then owns slot s and walks them,
//            acc += spfh[j][s] * w_j: per neighbour the wavefront reads
//            one contiguous 264-byte SPFH row (the traffic of the kernel: n * K * 264 bytes).  Block sums over 11 slots in ascending
//            slot order, through LDS.
// No float atomics and a fixed order in every sum: a point's two rows are the same bits alone, in any batch and across runs.
#include "common.h"

#define FPFH_DIM 33
#define FPFH_BINS 11
#define FPFH_WAVES 4
#define FPFH_MAX_NN 128

// bin of x in bin units: 0 if !(x >= 0) (NaN and -inf included), 10 if x >= 11 (+inf included), else (int)x
__device__ __forceinline__ int fpfh_bin(double x)
{
    if (!(x >= 0.0)) return 0;
    if (x >= (double)FPFH_BINS) return FPFH_BINS - 1;
    return (int)x;
}

// fp64 squared distance in the contract's order, from the fp32 coordinates promoted
__device__ __forceinline__ double fpfh_d2(const float* __restrict__ pts, size_t i, size_t j, double& dx, double& dy, double& dz)
{
    dx = (double)pts[3 * j] - (double)pts[3 * i];
    dy = (double)pts[3 * j + 1] - (double)pts[3 * i + 1];
    dz = (double)pts[3 * j + 2] - (double)pts[3 * i + 2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

// the three bins of the pair (i, j)
__device__ __forceinline__ void fpfh_pair_bins(const float* __restrict__ pts, const float* __restrict__ nrm, size_t i, size_t j, int bin[3])
{
    double dx, dy, dz;
    const double L = sqrt(fpfh_d2(pts, i, j, dx, dy, dz));
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if (L != 0.0) {                                              // (a NaN length goes on and ends in bin 0)
        double n1x = nrm[3 * i], n1y = nrm[3 * i + 1], n1z = nrm[3 * i + 2];
        double n2x = nrm[3 * j], n2y = nrm[3 * j + 1], n2z = nrm[3 * j + 2];
        const double a1 = dot3(n1x, n1y, n1z, dx, dy, dz) / L, a2 = dot3(n2x, n2y, n2z, dx, dy, dz) / L;
        f2 = a1;
        if (fabs(a1) < fabs(a2)) {                               // open3d: acos|a1| > acos|a2|
            double t;
            t = n1x; n1x = n2x; n2x = t;
            t = n1y; n1y = n2y; n2y = t;
            t = n1z; n1z = n2z; n2z = t;
            dx = -dx; dy = -dy; dz = -dz;
            f2 = -a2;
        }
        double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;      // v = d x n1
        const double vn = sqrt(dot3(vx, vy, vz, vx, vy, vz));
        if (vn == 0.0) {
            f2 = 0.0;
        } else {
            vx /= vn; vy /= vn; vz /= vn;
            const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;  // w = n1 x v
            f1 = dot3(vx, vy, vz, n2x, n2y, n2z);
            f0 = atan2(dot3(wx, wy, wz, n2x, n2y, n2z), dot3(n1x, n1y, n1z, n2x, n2y, n2z));
        }
    }
    const double pi = 3.141592653589793;
    bin[0] = fpfh_bin(11.0 * (f0 + pi) / (2.0 * pi));
    bin[1] = fpfh_bin(11.0 * (f1 + 1.0) / 2.0);
    bin[2] = fpfh_bin(11.0 * (f2 + 1.0) / 2.0);
}

__global__ void __launch_bounds__(FPFH_WAVES * WAVE) k_spfh(const float* __restrict__ pts, const float* __restrict__ nrm, int n,
                                                          const int* __restrict__ nbr, int k_nbr, int kmax,
                                                          double* __restrict__ spfh)
{
    __shared__ int cnt[FPFH_WAVES][FPFH_DIM];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const long long pi = (long long)blockIdx.x * FPFH_WAVES + wave;
    if (pi >= n) return;                                         // wave-uniform; the waves of a workgroup share no barrier
    const size_t i = (size_t)pi;
    if (lane < FPFH_DIM) cnt[wave][lane] = 0;
    wave_sync();
    const int* row = nbr + i * (size_t)k_nbr;
    int m = 0;
    for (int c0 = 0; c0 < kmax; c0 += WAVE) {
        const int c = c0 + lane;
        const int j = c < kmax ? row[c] : n;
        const bool valid = (unsigned int)j < (unsigned int)n;
        m += __popcll(__ballot(valid));
        if (valid && c > 0) {                                    // column 0 is the point itself
            int bin[3];
            fpfh_pair_bins(pts, nrm, i, (size_t)j, bin);
            atomicAdd(&cnt[wave][bin[0]], 1);
            atomicAdd(&cnt[wave][FPFH_BINS + bin[1]], 1);
            atomicAdd(&cnt[wave][2 * FPFH_BINS + bin[2]], 1);
        }
    }
    wave_sync();
    if (lane < FPFH_DIM) spfh[i * FPFH_DIM + lane] = m < 2 ? 0.0 : (double)cnt[wave][lane] * (100.0 / (double)(m - 1));
}

__global__ void __launch_bounds__(FPFH_WAVES * WAVE) k_fpfh(const float* __restrict__ pts, int n, const int* __restrict__ nbr, int k_nbr,
                                                          int kmax, const double* __restrict__ spfh, double* __restrict__ fpfh)
{
    __shared__ double wgt[FPFH_WAVES][FPFH_MAX_NN];
    __shared__ int col[FPFH_WAVES][FPFH_MAX_NN];
    __shared__ double accs[FPFH_WAVES][FPFH_DIM];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const long long pi = (long long)blockIdx.x * FPFH_WAVES + wave;
    if (pi >= n) return;
    const size_t i = (size_t)pi;
    const int* row = nbr + i * (size_t)k_nbr;
    int m = 0, nw = 0;                                           // row entries; weighted neighbours, compacted in column order
    for (int c0 = 0; c0 < kmax; c0 += WAVE) {                    // kmax <= FPFH_MAX_NN
        const int c = c0 + lane;
        const int j = c < kmax ? row[c] : n;
        const bool valid = (unsigned int)j < (unsigned int)n;
        m += __popcll(__ballot(valid));
        double w = 0.0;
        if (valid && c > 0) {                                    // column 0 is the point itself
            double dx, dy, dz;
            const double d2 = fpfh_d2(pts, i, (size_t)j, dx, dy, dz);
            if (d2 > 0.0 && d2 < __builtin_inf()) w = 1.0 / d2;     // duplicates, NaN and overflow carry no weight
        }
        const unsigned long long has = __ballot(w != 0.0);
        if (w != 0.0) {
            const int slot = nw + __popcll(has & ((1ull << lane) - 1ull));
            wgt[wave][slot] = w;
            col[wave][slot] = j;
        }
        nw += __popcll(has);
    }
    wave_sync();
    double acc = 0.0;
    if (lane < FPFH_DIM && m >= 2) {
#pragma unroll 4
        for (int c = 0; c < nw; c++) acc += spfh[(size_t)col[wave][c] * FPFH_DIM + lane] * wgt[wave][c];
        accs[wave][lane] = acc;
    }
    wave_sync();
    if (lane >= FPFH_DIM) return;
    double out = 0.0;
    if (m >= 2) {
        const int b0 = lane / FPFH_BINS * FPFH_BINS;
        double S = 0.0;
        for (int s = 0; s < FPFH_BINS; s++) S += accs[wave][b0 + s];
        if (S != 0.0) acc *= 100.0 / S;
        out = acc + spfh[i * FPFH_DIM + lane];
    }
    fpfh[i * FPFH_DIM + lane] = out;
}

extern "C" size_t buf_fpfh_ws_bytes(int n)
{
    if (n <= 0) return 0;
    return align_up((size_t)n * FPFH_DIM * sizeof(double), 256);
}

extern "C" int buf_fpfh(const float* pts, const float* normals, int n, const int* nbr, int k_nbr, int max_nn, double* fpfh_out,
                        double* spfh_out, void* ws, size_t ws_bytes, void* stream)
{
    BUF_REQUIRE(n >= 0 && k_nbr >= 1, BUF_EINVAL, "buf_fpfh: n=%d k_nbr=%d", n, k_nbr);
    BUF_REQUIRE(max_nn >= 2 && max_nn <= FPFH_MAX_NN, BUF_EINVAL, "buf_fpfh: max_nn=%d (2..%d)", max_nn, FPFH_MAX_NN);
    if (n == 0) return BUF_OK;
    BUF_REQUIRE(pts && normals && nbr, BUF_EINVAL, "buf_fpfh: null input");
    BUF_REQUIRE(fpfh_out, BUF_EINVAL, "buf_fpfh: null output");
    double* spfh = spfh_out;
    if (!spfh) {                                                 // the SPFH table then lives in the workspace
        const size_t need = buf_fpfh_ws_bytes(n);
        BUF_REQUIRE(ws && ws_bytes >= need, BUF_EINVAL, "buf_fpfh: workspace %zu < %zu bytes (no spfh_out given)", ws ? ws_bytes : (size_t)0, need);
        spfh = (double*)ws;
    }
    hipStream_t s = (hipStream_t)stream;
    const int kmax = max_nn < k_nbr ? max_nn : k_nbr;
    const int blocks = cdiv(n, FPFH_WAVES);
    TimedSpan span;                                               // (measurement aid, off by default: tools/fpfh_time.py)
    bool timed = timing_begin(s, &span, ((24.0 + 4.0 * k_nbr) + 24.0 * kmax + 264.0) * n, BUF_TIMED_SPFH);
    k_spfh<<<blocks, FPFH_WAVES * WAVE, 0, s>>>(pts, normals, n, nbr, k_nbr, kmax, spfh);
    if (timed) timing_end(s, &span);
    timed = timing_begin(s, &span, 264.0 * (double)n * kmax, BUF_TIMED_FPFH);
    k_fpfh<<<blocks, FPFH_WAVES * WAVE, 0, s>>>(pts, n, nbr, k_nbr, kmax, spfh, fpfh_out);
    if (timed) timing_end(s, &span);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
