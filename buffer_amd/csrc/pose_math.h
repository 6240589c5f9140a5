// The small fp64 routines of the batched pose estimators (icp.hip, vgicp.hip, fgr.hip, sc2.hip, clique.hip): ONE definition of
// each.  Call them, do not restate them: the library is built with -ffp-contract=off -fno-fast-math, so a second caller cannot
// change a result bit of the first, only the inliner's decisions (profiles/pose_math_refactor.md has the per-kernel figures).
// The scalar routines are __host__ __device__ so that a host program can run them against float64 references
// (tests/native/pose_math_host.cpp); a host compiler other than hipcc defines the two qualifiers away and sees no wavefront code.
#pragma once
#include <math.h>
#include <stddef.h>
#ifdef __HIPCC__
#include "common.h"
#endif

// ---- vectors ---------------------------------------------------------------------------------
__host__ __device__ static inline void cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ static inline bool unit3(double* a)
{
    const double l = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if (!(l > 0.0) || !isfinite(l)) return false;
    a[0] /= l; a[1] /= l; a[2] /= l;
    return true;
}

// a unit vector orthogonal to the unit vector u
__host__ __device__ static inline void any_orthogonal3(const double* u, double* o)
{
    const double e[3] = { fabs(u[0]) < 0.6 ? 1.0 : 0.0, fabs(u[0]) < 0.6 ? 0.0 : 1.0, 0.0 };
    cross3(u, e, o);
    unit3(o);
}

__host__ __device__ static inline bool finite9(const double* H)
{
    for (int k = 0; k < 9; k++)
        if (!isfinite(H[k])) return false;
    return true;
}

// ---- Kabsch ----------------------------------------------------------------------------------
// R maximising tr(R H) over proper rotations, H = sum w (p - pc)(q - qc)^T, both 3x3 row-major.  One-sided Jacobi on the columns
// of H (H V = U S), singular values sorted descending; with U3 = U1 x U2 and V3 = V1 x V2 the rotation V diag(1, 1, d) U^T of the
// det-corrected SVD (d = sign det(V U^T)) is [V1 V2 V1xV2][U1 U2 U1xU2]^T whatever the sign of the third pair.  false (R
// untouched) for H = 0.  A caller that may hold a non-finite H and wants R untouched then asks finite9(H) first.
__host__ __device__ static inline bool kabsch_rotation(const double* H, double* R)
{
    double A[3][3], V[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { A[r][c] = H[3 * r + c]; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; sweep++) {
        bool rotated = false;
        for (int pr = 0; pr < 3; pr++) {
            const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
            const double al = (A[0][i] * A[0][i] + A[1][i] * A[1][i]) + A[2][i] * A[2][i];
            const double be = (A[0][j] * A[0][j] + A[1][j] * A[1][j]) + A[2][j] * A[2][j];
            const double ga = (A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j];
            if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
            const double ze = (be - al) / (2.0 * ga);
            const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
            const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
            for (int k = 0; k < 3; k++) {
                const double ai = A[k][i], aj = A[k][j];
                A[k][i] = cs * ai - sn * aj; A[k][j] = sn * ai + cs * aj;
                const double vi = V[k][i], vj = V[k][j];
                V[k][i] = cs * vi - sn * vj; V[k][j] = sn * vi + cs * vj;
            }
            rotated = true;
        }
        if (!rotated) break;
    }
    double s[3];
    int o[3] = { 0, 1, 2 };
    for (int c = 0; c < 3; c++) s[c] = (A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c];
    for (int a = 0; a < 2; a++)                                               // descending, stable
        for (int c = 0; c < 2 - a; c++)
            if (s[o[c]] < s[o[c + 1]]) { const int t = o[c]; o[c] = o[c + 1]; o[c + 1] = t; }
    double U1[3], U2[3], U3[3], V1[3], V2[3], V3[3];
    for (int k = 0; k < 3; k++) { U1[k] = A[k][o[0]]; U2[k] = A[k][o[1]]; V1[k] = V[k][o[0]]; V2[k] = V[k][o[1]]; }
    if (!unit3(U1)) return false;                                            // H = 0: no rotation to find
    const double pj = (U1[0] * U2[0] + U1[1] * U2[1]) + U1[2] * U2[2];
    for (int k = 0; k < 3; k++) U2[k] -= pj * U1[k];
    if (!(s[o[1]] > 1e-28 * s[o[0]]) || !unit3(U2)) any_orthogonal3(U1, U2);  // rank 1: any completion
    cross3(U1, U2, U3);
    cross3(V1, V2, V3);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = (V1[r] * U1[c] + V2[r] * U2[c]) + V3[r] * U3[c];
    return true;
}

// ---- 6x6 step --------------------------------------------------------------------------------
// H x = -g by LDL^T without pivoting, H given as its upper triangle (21, row by row); false when the system is not positive
// definite or the solution is not finite
__host__ __device__ static inline bool solve6(const double* up, const double* g, double (&x)[6])
{
    double A[6][6], L[6][6], D[6], y[6];
    int k = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { A[r][c] = up[k]; A[c][r] = up[k]; k++; }
    for (int j = 0; j < 6; j++) {
        double d = A[j][j];
        for (int m = 0; m < j; m++) d -= L[j][m] * L[j][m] * D[m];
        if (!(d > 0.0) || !isfinite(d)) return false;
        D[j] = d;
        L[j][j] = 1.0;
        for (int i = j + 1; i < 6; i++) {
            double e = A[i][j];
            for (int m = 0; m < j; m++) e -= L[i][m] * L[j][m] * D[m];
            L[i][j] = e / d;
        }
    }
    for (int i = 0; i < 6; i++) {
        double e = -g[i];
        for (int m = 0; m < i; m++) e -= L[i][m] * y[m];
        y[i] = e;
    }
    for (int i = 5; i >= 0; i--) {
        double e = y[i] / D[i];
        for (int m = i + 1; m < 6; m++) e -= L[m][i] * x[m];
        x[i] = e;
    }
    for (int i = 0; i < 6; i++)
        if (!isfinite(x[i])) return false;
    return true;
}

// R = Rz(x2) Ry(x1) Rx(x0), row-major (open3d TransformVector6dToMatrix4d, restated); x3..5 is the translation
__host__ __device__ static inline void rot_zyx(const double* x, double* R)
{
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    R[0] = cg * cb; R[1] = cg * sb * sa - sg * ca; R[2] = cg * sb * ca + sg * sa;
    R[3] = sg * cb; R[4] = sg * sb * sa + cg * ca; R[5] = sg * sb * ca - cg * sa;
    R[6] = -sb;     R[7] = cb * sa;                R[8] = cb * ca;
}

// ---- Generalized ICP term ----------------------------------------------------------------------
// From S (upper triangle 00 01 02 11 12 22 of the summed covariances, symmetric positive definite), the moved point p and the
// residual d = p - q: M = S^-1 by cofactors and, with A = -[p]x (row r of M A is p x (row r of M), A^T x is p x x), the blocks of
// J^T M J and J^T M d for J = [A, I].  MA is formed once and serves all three.
struct GicpTerm { double Mm[3][3], MA[3][3], AtMA[3][3], Md[3], AtMd[3]; };

__host__ __device__ static inline void gicp_term(const double* S, const double* p, double dx, double dy, double dz, GicpTerm& t)
{
    const double c00 = S[3] * S[5] - S[4] * S[4], c01 = S[2] * S[4] - S[1] * S[5], c02 = S[1] * S[4] - S[2] * S[3];
    const double c11 = S[0] * S[5] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[4], c22 = S[0] * S[3] - S[1] * S[1];
    const double idet = 1.0 / ((S[0] * c00 + S[1] * c01) + S[2] * c02);
    const double Mm[3][3] = { { c00 * idet, c01 * idet, c02 * idet }, { c01 * idet, c11 * idet, c12 * idet },
                              { c02 * idet, c12 * idet, c22 * idet } };
    double col[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) t.Mm[r][c] = Mm[r][c];
        cross3(p, Mm[r], t.MA[r]);
        t.Md[r] = (Mm[r][0] * dx + Mm[r][1] * dy) + Mm[r][2] * dz;
    }
    for (int c = 0; c < 3; c++) {
        const double mc[3] = { t.MA[0][c], t.MA[1][c], t.MA[2][c] };
        cross3(p, mc, col);
        for (int r = 0; r < 3; r++) t.AtMA[r][c] = col[r];
    }
    cross3(p, t.Md, t.AtMd);
}

// row j of a normal array in fp64; zero (C = I) for a null array and for a row that is not a unit vector (| |n|^2 - 1 | >= 1e-3,
// or any component not finite: NaN and inf fail the comparison)
__host__ __device__ static inline void unit_normal_or_zero(const float* __restrict__ normals, size_t j, double (&n)[3])
{
    n[0] = 0.0; n[1] = 0.0; n[2] = 0.0;
    if (!normals) return;
    const double a = normals[3 * j], b = normals[3 * j + 1], c = normals[3 * j + 2];
    const double l2 = (a * a + b * b) + c * c;
    if (fabs(l2 - 1.0) < 1e-3) { n[0] = a; n[1] = b; n[2] = c; }
}

#ifdef __HIPCC__
// ---- fixed-order sums ------------------------------------------------------------------------
// sum over the wavefront by a xor butterfly, in every lane
template <typename T> __device__ __forceinline__ T wave_sum(T v)
{
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// sum of v over the WAVES wavefronts of the workgroup, wave butterfly then the waves one after the other through LDS; the result
// lands in out[0..NV) (threads 0..NV-1 store it).  v is left holding the wave sums.
template <int NV, int WAVES>
__device__ __forceinline__ void tile_sum(double (&v)[NV], double (*part)[NV], double* __restrict__ out)
{
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NV; k++)
        for (int d = WAVE / 2; d > 0; d >>= 1) v[k] += __shfl_xor(v[k], d, WAVE);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; k++) part[w][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = part[0][threadIdx.x];
        for (int j = 1; j < WAVES; j++) s += part[j][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// the same sum in place, the result in every thread (EVERY = false: in thread 0 alone, where no other thread reads it): wave
// butterfly, then (w0 + w1) + (w2 + w3) through red (WAVES * NV doubles)
template <int NV, int WAVES, bool EVERY = true>
__device__ __forceinline__ void tile_sum(double (&v)[NV], double* red)
{
    static_assert(WAVES == 4, "the tree over the wavefronts is written for four");
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
    for (int k = 0; k < NV; k++)
        for (int d = WAVE / 2; d > 0; d >>= 1) v[k] += __shfl_xor(v[k], d, WAVE);
    __syncthreads();                                             // red may still be read from the last use
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; k++) red[wave * NV + k] = v[k];
    __syncthreads();
    if (EVERY || threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; k++) v[k] = (red[k] + red[NV + k]) + (red[2 * NV + k] + red[3 * NV + k]);
}
#endif
