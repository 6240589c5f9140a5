// N13  Normals and covariances of radius / hybrid neighbourhoods (open3d estimate_normals / estimate_covariances with
// KDTreeSearchParamRadius / KDTreeSearchParamHybrid, restated from the published form, parity unpinned: the contract is in
// include/buffer_hip.h) on the sorted radius rows of buf_grid_query.
//
//   k_row_normals   one LANE per point (one wavefront per workgroup): the nine moments of a row are a sum in column order, which a
//                   single lane keeps in 18 VGPRs without any exchange (the wave-per-point layout of k_iss_saliency spends two LDS
//                   round trips per 64 columns on the same order: DESIGN 7a).  Slot t of the launch handles point order[t]: with the
//                   grid's cell order the 64 gathers of a column stay inside a few cells.
//                   NRM_ROWS_DIRECT: every lane reads its own row, column after column (a lane touches one 64-byte line per 16
//                   columns; the lines of the 64 rows are re-read from L1 / L2).
//                   NRM_ROWS_LDS:    the wavefront loads NRM_TILE columns of its 64 rows, two rows per load instruction (32 lanes x 4
//                   bytes = 128 bytes contiguous per row), into an LDS tile, and every lane then walks its tile row.
//                   Both read the same entries in the same order: the same bits.  The LDS tile is the default: 0.44 ms against 1.07 ms
//                   (3.5 M points, rows of 30) and 0.10 ms against 0.37 ms (0.67 M points) on an MI355X;
//                   BUF_N13_ROWS=direct|lds picks one for tools/normals_time.py.
// No float atomics, no workspace, nothing read back, a fixed order in every sum: a point's outputs are the same bits alone, in any batch,
// with any `order` and across runs.
#include "common.h"

#define NRM_TILE 32
#define NRM_ROWS_DIRECT 0
#define NRM_ROWS_LDS 1

template <int ROWS>
__global__ void __launch_bounds__(WAVE) k_row_normals(const float* __restrict__ pts, int n, const int* __restrict__ nbr, int k_nbr, int kmax,
                                                      const int* __restrict__ order, double cam_x, double cam_y, double cam_z, int orient,
                                                      float* __restrict__ normals, double* __restrict__ cov_out, int* __restrict__ count)
{
    const int lane = threadIdx.x;
    const long long t = (long long)blockIdx.x * WAVE + lane;
    int pi = -1;                                                 // -1: an idle lane (past n, or an `order` entry outside [0, n))
    if (t < n) {
        pi = order ? order[t] : (int)t;
        if ((unsigned int)pi >= (unsigned int)n) pi = -1;
    }
    const size_t i = pi < 0 ? 0 : (size_t)pi;
    const int* row = nbr + i * (size_t)k_nbr;
    const double qx = pi < 0 ? 0.0 : (double)pts[3 * i], qy = pi < 0 ? 0.0 : (double)pts[3 * i + 1], qz = pi < 0 ? 0.0 : (double)pts[3 * i + 2];
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    int m = 0;
#define NRM_ADD(j)                                                                                                                    \
    if ((unsigned int)(j) < (unsigned int)n) {                                                                                        \
        const size_t c_ = (size_t)(j);                                                                                                \
        const double dx = (double)pts[3 * c_] - qx, dy = (double)pts[3 * c_ + 1] - qy, dz = (double)pts[3 * c_ + 2] - qz;            \
        s1x += dx; s1y += dy; s1z += dz;                                                                                              \
        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;                              \
        m++;                                                                                                                          \
    }
    if constexpr (ROWS == NRM_ROWS_LDS) {
        __shared__ int tile[WAVE][NRM_TILE + 1];                 // + 1: lane l walks row l, the rows start in different banks
        const int half = lane / NRM_TILE, tc = lane % NRM_TILE;
        for (int c0 = 0; c0 < kmax; c0 += NRM_TILE) {            // (kmax is uniform: every lane runs every trip)
            const int w = kmax - c0 < NRM_TILE ? kmax - c0 : NRM_TILE;
            for (int r0 = 0; r0 < WAVE; r0 += WAVE / NRM_TILE) {
                const int r = r0 + half;
                const int pr = __shfl(pi, r);
                tile[r][tc] = (pr >= 0 && tc < w) ? nbr[(size_t)pr * (size_t)k_nbr + (size_t)(c0 + tc)] : -1;
            }
            wave_sync();
            if (pi >= 0)
                for (int c = 0; c < w; c++) {
                    const int j = tile[lane][c];
                    NRM_ADD(j)
                }
            wave_sync();
        }
    } else if (pi >= 0) {
        for (int c = 0; c < kmax; c++) {
            const int j = row[c];
            NRM_ADD(j)
        }
    }
#undef NRM_ADD
    if (pi < 0) return;
    double cov[6] = { 1.0, 0.0, 0.0, 1.0, 0.0, 1.0 };            // fewer than 3 points: open3d's identity
    double nrm[3] = { 0.0, 0.0, 1.0 };
    if (m >= 3) {
        const double dm = (double)m;
        const double mx = s1x / dm, my = s1y / dm, mz = s1z / dm;
        cov[0] = sxx / dm - mx * mx; cov[1] = sxy / dm - mx * my; cov[2] = sxz / dm - mx * mz;
        cov[3] = syy / dm - my * my; cov[4] = syz / dm - my * mz; cov[5] = szz / dm - mz * mz;
        bool finite = true;
        for (int e = 0; e < 6; e++) finite = finite && fabs(cov[e]) < __builtin_inf();
        if (finite) {
            o3d_fast_eigen3x3(cov, nrm);
            if (nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2] == 0.0) { nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0; }   // EstimateNormals
        } else {                                                 // a hand-made row that names a non-finite point
            nrm[0] = nrm[1] = nrm[2] = __builtin_nan("");
        }
    }
    if (orient) {                                                // OrientNormalsTowardsCameraLocation, as k_knn_normals
        const double rx = cam_x - qx, ry = cam_y - qy, rz = cam_z - qz;
        if (nrm[0] * rx + nrm[1] * ry + nrm[2] * rz < 0.0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
    }
    if (normals) { normals[3 * i] = (float)nrm[0]; normals[3 * i + 1] = (float)nrm[1]; normals[3 * i + 2] = (float)nrm[2]; }
    if (cov_out)
        for (int e = 0; e < 6; e++) cov_out[6 * i + e] = cov[e];
    if (count) count[i] = m;
}

extern "C" int buf_row_normals(const float* pts, int n, const int* nbr, int k_nbr, int max_nn, const int* order, const double* camera_host,
                               int orient, float* normals_out, double* cov_out, int* count_out, void* stream)
{
    BUF_REQUIRE(n >= 0, BUF_EINVAL, "buf_row_normals: n=%d", n);
    BUF_REQUIRE(k_nbr >= 1, BUF_EINVAL, "buf_row_normals: k_nbr=%d", k_nbr);
    BUF_REQUIRE(max_nn >= 0, BUF_EINVAL, "buf_row_normals: max_nn=%d", max_nn);
    BUF_REQUIRE(normals_out || cov_out || count_out, BUF_EINVAL, "buf_row_normals: null outputs normals_out, cov_out and count_out");
    BUF_REQUIRE(!orient || camera_host, BUF_EINVAL, "buf_row_normals: null camera_host with orient=%d", orient);
    if (n == 0) return BUF_OK;
    BUF_REQUIRE(pts, BUF_EINVAL, "buf_row_normals: null input pts");
    BUF_REQUIRE(nbr, BUF_EINVAL, "buf_row_normals: null input nbr");
    const int kmax = max_nn && max_nn < k_nbr ? max_nn : k_nbr;
    const double cx = orient ? camera_host[0] : 0.0, cy = orient ? camera_host[1] : 0.0, cz = orient ? camera_host[2] : 0.0;
    const char* rows = getenv("BUF_N13_ROWS");                   // development switch (tools/normals_time.py): direct | lds
    const bool lds = rows ? strcmp(rows, "direct") != 0 : true;
    hipStream_t s = (hipStream_t)stream;
    if (lds)
        k_row_normals<NRM_ROWS_LDS><<<cdiv(n, WAVE), WAVE, 0, s>>>(pts, n, nbr, k_nbr, kmax, order, cx, cy, cz, orient, normals_out, cov_out, count_out);
    else
        k_row_normals<NRM_ROWS_DIRECT><<<cdiv(n, WAVE), WAVE, 0, s>>>(pts, n, nbr, k_nbr, kmax, order, cx, cy, cz, orient, normals_out, cov_out, count_out);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
