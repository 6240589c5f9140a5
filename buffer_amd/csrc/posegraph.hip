// N5  Pose-graph optimisation with line processes (Choi et al. 2015), G graphs per call: the contract is the comment of
// buf_pose_graph_optimize in include/buffer_hip.h.  All arithmetic fp64, no FMA (-ffp-contract=off), no float atomics.
//
//   k_pose_graph   ONE launch per call, one workgroup of PG_THREADS per graph runs the whole Levenberg-Marquardt loop (the model of
//                  k_post_refine: nothing is read back, nothing synchronises with the host; the loop is bounded by max_iterations).
//     linearise    one thread per edge: residual, q, l, the two Jacobians -> ONE record per edge (PG_REC doubles):
//                  l J_i^T L J_i, l J_j^T L J_j, l J_i^T L J_j, l J_i^T L r, l J_j^T L r, q, l (L = the edge's information matrix)
//     assemble     one thread per (free node, row a, column b | gradient): the node's row of H and g gathered over its incident
//                  edges in ascending edge order (per-node adjacency built on the host)
//     factor       H + lambda I copied to a second dense square and factored in place: right-looking blocked Cholesky, block PG_NB;
//                  the diagonal block is factored in LDS by one thread, the panel below it is solved one row per thread and kept
//                  in LDS [PG_NB][rows], the trailing update runs 4x4 register tiles of the lower triangle from that panel
//     solve        blocked forward / backward substitution with the right-hand side in LDS
//     sums         every sum over edges or unknowns is a strided per-thread partial (i, i + PG_THREADS, ...) and a binary tree over
//                  the PG_THREADS partials in LDS: a fixed shape for a given length
// Every thread of the workgroup holds the same loop state (all scalars come out of workgroup reductions), so control flow is uniform.
#include "common.h"

#define PG_THREADS 256
#define PG_NB 8
#define PG_MAXD (6 * (BUF_PG_MAX_NODES - 1))
#define PG_PANEL_ROWS 768                        // >= PG_MAXD - 1 + 3 (the 4x4 tiles read up to 3 rows past the panel)
#define PG_REC 128                               // doubles per edge record
#define PG_R_HII 0
#define PG_R_HJJ 36
#define PG_R_HIJ 72
#define PG_R_GI 108
#define PG_R_GJ 114
#define PG_R_Q 120
#define PG_R_L 121
#define PG_TICKS 4                               // per graph: loop ticks, factorisation ticks, solve ticks, linearise + assemble ticks

struct PgArgs {
    const double* mu; const int* node_off; const int* edge_off; const int* fixed; const int* edge_i; const int* edge_j; const int* unc;
    const int* adj_ptr; const int* adj;
    const double* Z; const double* info; const double* X0;
    double* X; int* status; double* cost; double* edge_out;
    double* rec; double* cbuf; double* Xc; double* H; double* L; double* vec; long long* ticks;
    int max_nodes, max_iter;
    double eps_step, eps_cost, tau0;
};

struct PgLds {
    double panel[PG_NB][PG_PANEL_ROWS];
    double red[PG_THREADS];
    double rhs[PG_PANEL_ROWS];
    double dblk[PG_NB][PG_NB + 1];
    int flag;
};

// c = a^T b, c = a b (3x3 row-major), each entry (x0*y0 + x1*y1) + x2*y2
__device__ __forceinline__ void pg_mul_tn(const double* a, const double* b, double* c)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) c[3 * r + k] = (a[r] * b[k] + a[3 + r] * b[3 + k]) + a[6 + r] * b[6 + k];
}
__device__ __forceinline__ void pg_mul_nn(const double* a, const double* b, double* c)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) c[3 * r + k] = (a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k]) + a[3 * r + 2] * b[6 + k];
}
__device__ __forceinline__ void pg_tvec(const double* a, const double* v, double* o)      // o = a^T v
{
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = (a[r] * v[0] + a[3 + r] * v[1]) + a[6 + r] * v[2];
}
__device__ __forceinline__ void pg_vec(const double* a, const double* v, double* o)       // o = a v
{
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = (a[3 * r] * v[0] + a[3 * r + 1] * v[1]) + a[3 * r + 2] * v[2];
}

// Log of a rotation through its quaternion (Shepperd's branch on the largest of w, x, y, z) and atan2: a few ulp on [0, pi]
__device__ __forceinline__ void pg_log(const double* R, double* phi)
{
    double w, x, y, z;
    const double tr = (R[0] + R[4]) + R[8];
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(tr + 1.0);
        w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2.0 * sqrt(((1.0 + R[0]) - R[4]) - R[8]);
        w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2.0 * sqrt(((1.0 + R[4]) - R[0]) - R[8]);
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(((1.0 + R[8]) - R[0]) - R[4]);
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
    }
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double nv = sqrt((x * x + y * y) + z * z);
    const double k = nv > 0.0 ? 2.0 * atan2(nv, w) / nv : 2.0;
    phi[0] = k * x; phi[1] = k * y; phi[2] = k * z;
}

// Exp(a) = I + A [a]x + B [a]x^2, A = sin(t)/t, B = (sin(t/2)/(t/2))^2 / 2, t = |a| (A = 1, B = 1/2 at t = 0)
__device__ __forceinline__ void pg_exp(const double* a, double* R)
{
    const double t2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double t = sqrt(t2);
    double A = 1.0, B = 0.5;
    if (t > 0.0) {
        const double h = sin(0.5 * t) / (0.5 * t);
        A = sin(t) / t;
        B = 0.5 * (h * h);
    }
    R[0] = 1.0 - B * (a[1] * a[1] + a[2] * a[2]);
    R[4] = 1.0 - B * (a[0] * a[0] + a[2] * a[2]);
    R[8] = 1.0 - B * (a[0] * a[0] + a[1] * a[1]);
    R[1] = B * (a[0] * a[1]) - A * a[2];
    R[3] = B * (a[0] * a[1]) + A * a[2];
    R[2] = B * (a[0] * a[2]) + A * a[1];
    R[6] = B * (a[0] * a[2]) - A * a[1];
    R[5] = B * (a[1] * a[2]) - A * a[0];
    R[7] = B * (a[1] * a[2]) + A * a[0];
}

__device__ __forceinline__ void pg_pose(const double* X, double* R, double* p)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        R[3 * r] = X[4 * r]; R[3 * r + 1] = X[4 * r + 1]; R[3 * r + 2] = X[4 * r + 2];
        p[r] = X[4 * r + 3];
    }
}

// residual of one edge: r = [Log(R_E); t_E], E = Z^-1 X_i^-1 X_j; also R_E and M = X_j^-1 X_i
__device__ __forceinline__ void pg_residual(const double* Xi, const double* Xj, const double* Z, double* r, double* RE, double* RM, double* pM)
{
    double Ri[9], Rj[9], RZ[9], pi[3], pj[3], tZ[3], RA[9], d[3], tA[3], e[3];
    pg_pose(Xi, Ri, pi); pg_pose(Xj, Rj, pj); pg_pose(Z, RZ, tZ);
    pg_mul_tn(Rj, Ri, RM);
    d[0] = pi[0] - pj[0]; d[1] = pi[1] - pj[1]; d[2] = pi[2] - pj[2];
    pg_tvec(Rj, d, pM);
    pg_mul_tn(Ri, Rj, RA);
    d[0] = pj[0] - pi[0]; d[1] = pj[1] - pi[1]; d[2] = pj[2] - pi[2];
    pg_tvec(Ri, d, tA);
    pg_mul_tn(RZ, RA, RE);
    e[0] = tA[0] - tZ[0]; e[1] = tA[1] - tZ[1]; e[2] = tA[2] - tZ[2];
    pg_tvec(RZ, e, r + 3);
    pg_log(RE, r);
}

// q = r^T L r with Lr = L r, each row ((((l0 r0 + l1 r1) + l2 r2) + l3 r3) + l4 r4) + l5 r5
__device__ __forceinline__ double pg_quad(const double* __restrict__ info, const double* r, double* Lr)
{
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double s = info[6 * a] * r[0];
#pragma unroll
        for (int b = 1; b < 6; b++) s += info[6 * a + b] * r[b];
        Lr[a] = s;
    }
#pragma unroll
    for (int a = 0; a < 6; a++) q += r[a] * Lr[a];
    return q;
}

__device__ __forceinline__ double pg_weight(double q, double mu, int robust)
{
    if (!robust) return 1.0;
    const double s = mu / (mu + q);
    return s * s;
}
__device__ __forceinline__ double pg_cost(double q, double mu, int robust) { return robust ? mu * q / (mu + q) : q; }

// out[x][y] = l * sum_a Ja[a][x] * B[a][y] (6x6), ascending a
__device__ __forceinline__ void pg_jtb(const double* Ja, const double* B, double l, double* __restrict__ out, bool transpose_out)
{
#pragma unroll
    for (int x = 0; x < 6; x++)
#pragma unroll
        for (int y = 0; y < 6; y++) {
            double s = Ja[x] * B[y];
#pragma unroll
            for (int a = 1; a < 6; a++) s += Ja[6 * a + x] * B[6 * a + y];
            out[transpose_out ? 6 * y + x : 6 * x + y] = l * s;
        }
}
__device__ __forceinline__ void pg_lj(const double* __restrict__ info, const double* J, double* B)      // B = L J
{
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int y = 0; y < 6; y++) {
            double s = info[6 * a] * J[y];
#pragma unroll
            for (int b = 1; b < 6; b++) s += info[6 * a + b] * J[6 * b + y];
            B[6 * a + y] = s;
        }
}

// one edge's record at the poses X (graph-local rows of 16); returns the edge's cost term
__device__ __noinline__ double pg_linearise_edge(const double* __restrict__ X, int i, int j, const double* __restrict__ Z,
                                                 const double* __restrict__ info, double mu, int robust, double* __restrict__ rec)
{
    double r[6], RE[9], RM[9], pM[3], Lr[6], Ji[36], Jj[36], B[36];
    pg_residual(X + 16 * i, X + 16 * j, Z, r, RE, RM, pM);
    const double q = pg_quad(info, r, Lr);
    const double l = pg_weight(q, mu, robust);
    // Jri = I + P/2 + P^2/12, P = [phi]x
    double Jri[9];
    {
        const double a = r[0], b = r[1], c = r[2];
        Jri[0] = 1.0 - (b * b + c * c) / 12.0; Jri[4] = 1.0 - (a * a + c * c) / 12.0; Jri[8] = 1.0 - (a * a + b * b) / 12.0;
        Jri[1] = (a * b) / 12.0 - 0.5 * c; Jri[3] = (a * b) / 12.0 + 0.5 * c;
        Jri[2] = (a * c) / 12.0 + 0.5 * b; Jri[6] = (a * c) / 12.0 - 0.5 * b;
        Jri[5] = (b * c) / 12.0 - 0.5 * a; Jri[7] = (b * c) / 12.0 + 0.5 * a;
    }
    double JM[9], RERM[9], PX[9], PXRM[9], T3[9];
    pg_mul_nn(Jri, RM, JM);
    pg_mul_nn(RE, RM, RERM);
    PX[0] = 0.0; PX[1] = -pM[2]; PX[2] = pM[1]; PX[3] = pM[2]; PX[4] = 0.0; PX[5] = -pM[0]; PX[6] = -pM[1]; PX[7] = pM[0]; PX[8] = 0.0;
    pg_mul_nn(PX, RM, PXRM);
    pg_mul_nn(RE, PXRM, T3);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            Ji[6 * a + b] = -JM[3 * a + b];  Ji[6 * a + 3 + b] = 0.0;
            Ji[6 * (a + 3) + b] = -T3[3 * a + b];  Ji[6 * (a + 3) + 3 + b] = -RERM[3 * a + b];
            Jj[6 * a + b] = Jri[3 * a + b];  Jj[6 * a + 3 + b] = 0.0;
            Jj[6 * (a + 3) + b] = 0.0;  Jj[6 * (a + 3) + 3 + b] = RE[3 * a + b];
        }
    pg_lj(info, Ji, B);
    pg_jtb(Ji, B, l, rec + PG_R_HII, false);
    pg_lj(info, Jj, B);
    pg_jtb(Jj, B, l, rec + PG_R_HJJ, false);
    pg_jtb(Ji, B, l, rec + PG_R_HIJ, false);
#pragma unroll
    for (int x = 0; x < 6; x++) {
        double si = Ji[x] * Lr[0], sj = Jj[x] * Lr[0];
#pragma unroll
        for (int a = 1; a < 6; a++) { si += Ji[6 * a + x] * Lr[a]; sj += Jj[6 * a + x] * Lr[a]; }
        rec[PG_R_GI + x] = l * si;
        rec[PG_R_GJ + x] = l * sj;
    }
    rec[PG_R_Q] = q;
    rec[PG_R_L] = l;
    return pg_cost(q, mu, robust);
}

// fixed-shape sum of v[0..n): strided partials, then a binary tree over the PG_THREADS partials
__device__ __forceinline__ double pg_block_sum(const double* __restrict__ v, int n, double* red)
{
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += PG_THREADS) s += v[i];
    red[tid] = s;
    __syncthreads();
    for (int st = PG_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}
__device__ __forceinline__ double pg_block_max(double m, double* red)      // NaN-propagating: a NaN partial makes the result NaN
{
    const int tid = threadIdx.x;
    red[tid] = m;
    __syncthreads();
    for (int st = PG_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            const double a = red[tid], b = red[tid + st];
            red[tid] = (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b);
        }
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

struct PgGraph {
    int n, ne, fixed, nfree, D, robust;
    double mu;
    const int* ei; const int* ej; const int* unc; const int* adj_ptr; const int* adj;
    const double* Z; const double* info;
    double* rec; double* cbuf; double* H; double* L; double* g; double* delta; double* tmp;
};

__device__ __forceinline__ void pg_linearise(const PgGraph& G, const double* X)
{
    for (int e = threadIdx.x; e < G.ne; e += PG_THREADS)
        G.cbuf[e] = pg_linearise_edge(X, G.ei[e], G.ej[e], G.Z + 16 * (size_t)e, G.info + 36 * (size_t)e, G.mu, G.robust && G.unc[e],
                                      G.rec + PG_REC * (size_t)e);
    __syncthreads();
}

// cost terms only (candidate poses, and the edge outputs at the end: out2 != nullptr -> (l, q) per edge)
__device__ __forceinline__ void pg_costs(const PgGraph& G, const double* X, double* out2)
{
    for (int e = threadIdx.x; e < G.ne; e += PG_THREADS) {
        double r[6], RE[9], RM[9], pM[3], Lr[6];
        pg_residual(X + 16 * G.ei[e], X + 16 * G.ej[e], G.Z + 16 * (size_t)e, r, RE, RM, pM);
        const double q = pg_quad(G.info + 36 * (size_t)e, r, Lr);
        const int rb = G.robust && G.unc[e];
        G.cbuf[e] = pg_cost(q, G.mu, rb);
        if (out2) { out2[2 * (size_t)e] = pg_weight(q, G.mu, rb); out2[2 * (size_t)e + 1] = q; }
    }
    __syncthreads();
}

__device__ __forceinline__ void pg_assemble(const PgGraph& G)
{
    const int D = G.D;
    for (int i = threadIdx.x; i < D * D; i += PG_THREADS) G.H[i] = 0.0;
    __syncthreads();
    for (int w = threadIdx.x; w < G.nfree * 42; w += PG_THREADS) {
        const int fk = w / 42, rem = w - 42 * fk, a = rem / 7, b = rem - 7 * a;
        const int k = fk < G.fixed ? fk : fk + 1;
        double acc = 0.0;
        for (int p = G.adj_ptr[k]; p < G.adj_ptr[k + 1]; p++) {
            const int code = G.adj[p], e = code >> 1, side = code & 1;
            const double* rec = G.rec + PG_REC * (size_t)e;
            if (b == 6) { acc += rec[(side ? PG_R_GJ : PG_R_GI) + a]; continue; }
            acc += rec[(side ? PG_R_HJJ : PG_R_HII) + 6 * a + b];
            const int o = side ? G.ei[e] : G.ej[e];
            if (o == G.fixed) continue;
            const int fo = o < G.fixed ? o : o - 1;
            G.H[(size_t)(6 * fk + a) * D + 6 * fo + b] += rec[PG_R_HIJ + (side ? 6 * b + a : 6 * a + b)];
        }
        if (b == 6) G.g[6 * fk + a] = acc;
        else G.H[(size_t)(6 * fk + a) * D + 6 * fk + b] = acc;
    }
    __syncthreads();
}

__device__ __forceinline__ void pg_load_diag(PgLds& S, const double* __restrict__ L, int D, int kb, int nb)
{
    const int tid = threadIdx.x;
    if (tid < nb * nb) {
        const int r = tid / nb, c = tid - nb * r;
        if (c <= r) S.dblk[r][c] = L[(size_t)(kb + r) * D + kb + c];
    }
    __syncthreads();
}

// in-place lower Cholesky of the D x D row-major square L (its lower triangle); false on a pivot that is not positive and finite
__device__ __forceinline__ bool pg_cholesky(PgLds& S, double* __restrict__ L, int D)
{
    const int tid = threadIdx.x;
    if (tid == 0) S.flag = 0;
    for (int kb = 0; kb < D; kb += PG_NB) {
        const int nb = D - kb < PG_NB ? D - kb : PG_NB;
        const int m = D - kb - nb;
        pg_load_diag(S, L, D, kb, nb);
        if (tid == 0) {
            for (int j = 0; j < nb; j++) {
                double d = S.dblk[j][j];
                for (int k = 0; k < j; k++) d -= S.dblk[j][k] * S.dblk[j][k];
                if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) { S.flag = 1; d = 1.0; }
                d = sqrt(d);
                S.dblk[j][j] = d;
                for (int i = j + 1; i < nb; i++) {
                    double s = S.dblk[i][j];
                    for (int k = 0; k < j; k++) s -= S.dblk[i][k] * S.dblk[j][k];
                    S.dblk[i][j] = s / d;
                }
            }
        }
        __syncthreads();
        if (S.flag) return false;                                   // uniform: read after the barrier, never cleared inside the loop
        if (tid < nb * nb) {
            const int r = tid / nb, c = tid - nb * r;
            if (c <= r) L[(size_t)(kb + r) * D + kb + c] = S.dblk[r][c];
        }
        for (int rr = tid; rr < m; rr += PG_THREADS) {              // panel: row (kb + nb + rr) times the inverse transpose of the block
            double* row = L + (size_t)(kb + nb + rr) * D + kb;
            double x[PG_NB];
#pragma unroll
            for (int c = 0; c < PG_NB; c++) {
                if (c < nb) {
                    double s = row[c];
#pragma unroll
                    for (int k = 0; k < c; k++) s -= x[k] * S.dblk[c][k];
                    x[c] = s / S.dblk[c][c];
                    row[c] = x[c];
                    S.panel[c][rr] = x[c];
                } else {
                    x[c] = 0.0;
                }
            }
        }
        __syncthreads();
        const int nt = (m + 3) >> 2, ntri = nt * (nt + 1) / 2;      // 4x4 tiles of the lower triangle of the trailing m x m square
        for (int idx = tid; idx < ntri; idx += PG_THREADS) {
            int tr = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
            while (tr * (tr + 1) / 2 > idx) tr--;
            while ((tr + 1) * (tr + 2) / 2 <= idx) tr++;
            const int tc = idx - tr * (tr + 1) / 2;
            double acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
            for (int k = 0; k < nb; k++) {
                double a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; i++) { a[i] = S.panel[k][4 * tr + i]; b[i] = S.panel[k][4 * tc + i]; }
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] += a[i] * b[j];
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int rr = 4 * tr + i, cc = 4 * tc + j;
                    if (rr < m && cc <= rr) L[(size_t)(kb + nb + rr) * D + kb + nb + cc] -= acc[i][j];
                }
        }
        __syncthreads();
    }
    return true;
}

// S.rhs <- (L L^T)^-1 S.rhs
__device__ __forceinline__ void pg_solve(PgLds& S, const double* __restrict__ L, int D)
{
    const int tid = threadIdx.x;
    for (int kb = 0; kb < D; kb += PG_NB) {
        const int nb = D - kb < PG_NB ? D - kb : PG_NB;
        pg_load_diag(S, L, D, kb, nb);
        if (tid == 0)
            for (int c = 0; c < nb; c++) {
                double s = S.rhs[kb + c];
                for (int k = 0; k < c; k++) s -= S.dblk[c][k] * S.rhs[kb + k];
                S.rhs[kb + c] = s / S.dblk[c][c];
            }
        __syncthreads();
        for (int r = kb + nb + tid; r < D; r += PG_THREADS) {
            double s = S.rhs[r];
            for (int c = 0; c < nb; c++) s -= L[(size_t)r * D + kb + c] * S.rhs[kb + c];
            S.rhs[r] = s;
        }
        __syncthreads();
    }
    for (int kb = ((D - 1) / PG_NB) * PG_NB; kb >= 0; kb -= PG_NB) {
        const int nb = D - kb < PG_NB ? D - kb : PG_NB;
        pg_load_diag(S, L, D, kb, nb);
        if (tid == 0)
            for (int c = nb - 1; c >= 0; c--) {
                double s = S.rhs[kb + c];
                for (int k = nb - 1; k > c; k--) s -= S.dblk[k][c] * S.rhs[kb + k];
                S.rhs[kb + c] = s / S.dblk[c][c];
            }
        __syncthreads();
        for (int r = tid; r < kb; r += PG_THREADS) {
            double s = S.rhs[r];
            for (int c = nb - 1; c >= 0; c--) s -= L[(size_t)(kb + c) * D + r] * S.rhs[kb + c];
            S.rhs[r] = s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PG_THREADS) k_pose_graph(PgArgs A)
{
    __shared__ PgLds S;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n0 = A.node_off[g], e0 = A.edge_off[g];
    PgGraph G;
    G.n = A.node_off[g + 1] - n0;
    G.ne = A.edge_off[g + 1] - e0;
    G.fixed = A.fixed[g];
    G.mu = A.mu[g];
    G.robust = G.mu > 0.0;
    G.nfree = G.n > 0 ? G.n - 1 : 0;
    G.D = 6 * G.nfree;
    G.ei = A.edge_i + e0; G.ej = A.edge_j + e0; G.unc = A.unc + e0;
    G.adj_ptr = A.adj_ptr + n0 + g;                                 // every graph owns n + 1 row pointers, local to its adj slice
    G.adj = A.adj + 2 * (size_t)e0;
    G.Z = A.Z + 16 * (size_t)e0; G.info = A.info + 36 * (size_t)e0;
    G.rec = A.rec + PG_REC * (size_t)e0; G.cbuf = A.cbuf + e0;
    const size_t dm = (size_t)6 * (A.max_nodes > 1 ? A.max_nodes - 1 : 1);
    G.H = A.H + (size_t)g * dm * dm; G.L = A.L + (size_t)g * dm * dm;
    G.g = A.vec + (size_t)g * 3 * dm; G.delta = G.g + dm; G.tmp = G.delta + dm;
    const double* X0 = A.X0 + 16 * (size_t)n0;
    double* X = A.X + 16 * (size_t)n0;
    double* Xc = A.Xc + 16 * (size_t)n0;
    double* eout = A.edge_out + 2 * (size_t)e0;
    long long* ticks = A.ticks + PG_TICKS * (size_t)g;
    const int D = G.D;

    if (tid == 0) S.flag = 0;
    __syncthreads();
    int bad = 0;
    for (int i = tid; i < 16 * G.ne; i += PG_THREADS) bad |= !isfinite(G.Z[i]);
    for (int i = tid; i < 36 * G.ne; i += PG_THREADS) bad |= !isfinite(G.info[i]);
    for (int i = tid; i < 16 * G.n; i += PG_THREADS) { const double v = X0[i]; bad |= !isfinite(v); X[i] = v; }
    if (bad) S.flag = 1;
    __syncthreads();
    const int failed = S.flag;
    __syncthreads();
    if (failed) {
        const double nan = __builtin_nan("");
        for (int e = tid; e < G.ne; e += PG_THREADS) { eout[2 * (size_t)e] = nan; eout[2 * (size_t)e + 1] = nan; }
        if (tid == 0) {
            A.status[3 * g] = BUF_PG_FAILED; A.status[3 * g + 1] = 0; A.status[3 * g + 2] = 0;
            A.cost[2 * g] = nan; A.cost[2 * g + 1] = nan;
            for (int c = 0; c < PG_TICKS; c++) ticks[c] = 0;
        }
        return;
    }
    long long t_fac = 0, t_sol = 0, t_lin = 0;
    const long long t_begin = wall_clock64();
    pg_linearise(G, X);
    double F = pg_block_sum(G.cbuf, G.ne, S.red);
    const double F0 = F;
    int status = BUF_PG_NOTHING, solves = 0, accepted = 0;
    if (G.nfree > 0 && G.ne > 0) {
        pg_assemble(G);
        double md = -1.7976931348623157e308;
        for (int i = tid; i < D; i += PG_THREADS) { const double v = G.H[(size_t)i * D + i]; md = (v != v) ? v : (md != md ? md : (v > md ? v : md)); }
        const double lam0 = A.tau0 * pg_block_max(md, S.red);
        t_lin += wall_clock64() - t_begin;
        if (lam0 > 0.0) {
            double lam = lam0, nu = 2.0;
            status = BUF_PG_MAX_ITER;
            for (int it = 0; it < A.max_iter; it++) {
                solves++;
                long long t0 = wall_clock64();
                for (int i = tid; i < D * D; i += PG_THREADS) {
                    const int r = i / D, c = i - r * D;
                    if (c <= r) G.L[i] = c == r ? G.H[i] + lam : G.H[i];
                }
                __syncthreads();
                const bool ok = pg_cholesky(S, G.L, D);
                __syncthreads();
                t_fac += wall_clock64() - t0;
                bool accept = false;
                if (ok) {
                    t0 = wall_clock64();
                    for (int i = tid; i < D; i += PG_THREADS) S.rhs[i] = -G.g[i];
                    __syncthreads();
                    pg_solve(S, G.L, D);
                    double mx = 0.0;
                    for (int i = tid; i < D; i += PG_THREADS) {
                        const double d = S.rhs[i], ad = fabs(d);
                        G.delta[i] = d;
                        G.tmp[i] = d * (lam * d - G.g[i]);
                        mx = (ad != ad) ? ad : (mx != mx ? mx : (ad > mx ? ad : mx));
                    }
                    __syncthreads();
                    const double maxd = pg_block_max(mx, S.red);
                    t_sol += wall_clock64() - t0;
                    if (maxd <= A.eps_step) { status = BUF_PG_CONVERGED_STEP; break; }
                    for (int k = tid; k < G.n; k += PG_THREADS) {                       // candidate X' = X (Exp(a), b)
                        const double* x = X + 16 * k;
                        double* y = Xc + 16 * k;
                        if (k == G.fixed) {
                            for (int c = 0; c < 16; c++) y[c] = x[c];
                            continue;
                        }
                        const int fk = k < G.fixed ? k : k - 1;
                        double R[9], p[3], Ea[9], Rn[9], Rb[3];
                        pg_pose(x, R, p);
                        pg_exp(G.delta + 6 * fk, Ea);
                        pg_mul_nn(R, Ea, Rn);
                        pg_vec(R, G.delta + 6 * fk + 3, Rb);
                        for (int r = 0; r < 3; r++) {
                            y[4 * r] = Rn[3 * r]; y[4 * r + 1] = Rn[3 * r + 1]; y[4 * r + 2] = Rn[3 * r + 2];
                            y[4 * r + 3] = p[r] + Rb[r];
                        }
                        y[12] = 0.0; y[13] = 0.0; y[14] = 0.0; y[15] = 1.0;
                    }
                    __syncthreads();
                    pg_costs(G, Xc, nullptr);
                    const double Fp = pg_block_sum(G.cbuf, G.ne, S.red);
                    const double den = pg_block_sum(G.tmp, D, S.red);
                    const double rho = (F - Fp) / den;
                    if (rho > 0.0 && fabs(Fp) <= 1.7976931348623157e308) {
                        accept = true;
                        accepted++;
                        for (int i = tid; i < 16 * G.n; i += PG_THREADS) X[i] = Xc[i];
                        __syncthreads();
                        const double dF = F - Fp, Fold = F, c = 2.0 * rho - 1.0, f = 1.0 - (c * c) * c;
                        F = Fp;
                        lam = lam * (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
                        nu = 2.0;
                        if (dF <= A.eps_cost * Fold) { status = BUF_PG_CONVERGED_COST; break; }
                        if (it + 1 < A.max_iter) {
                            t0 = wall_clock64();
                            pg_linearise(G, X);
                            pg_assemble(G);
                            t_lin += wall_clock64() - t0;
                        }
                    }
                }
                if (!accept) {
                    lam = lam * nu;
                    nu = 2.0 * nu;
                    if (lam > 1e30 * lam0) { status = BUF_PG_STALLED; break; }
                }
            }
        }
    }
    pg_costs(G, X, eout);
    if (tid == 0) {
        A.status[3 * g] = status; A.status[3 * g + 1] = solves; A.status[3 * g + 2] = accepted;
        A.cost[2 * g] = F0; A.cost[2 * g + 1] = F;
        ticks[0] = wall_clock64() - t_begin; ticks[1] = t_fac; ticks[2] = t_sol; ticks[3] = t_lin;
    }
}

// ------------------------------------------------------------------------------------------
// the int region of a call: [mu as G int pairs | node_off (G + 1) | edge_off (G + 1) | fixed (G) | edge_i (E) | edge_j (E) |
// uncertain (E) | adj_ptr (N + G) | adj (2 E)], uploaded by upload_ints (pairstats.hip)
struct PgWs { int* meta; size_t meta_ints; double* rec; double* cbuf; double* Xc; double* H; double* L; double* vec; long long* ticks; };

static PgWs carve_pose_graph(WsCarver& w, int G, int N, int E, int max_nodes)
{
    PgWs p;
    const size_t dm = (size_t)6 * (max_nodes > 1 ? max_nodes - 1 : 1);
    p.ticks = w.take<long long>((size_t)PG_TICKS * G);                // first: tools/posegraph_time.py reads it from the workspace's start
    p.meta_ints = 2 * (size_t)G + 2 * ((size_t)G + 1) + (size_t)G + 3 * (size_t)E + ((size_t)N + G) + 2 * (size_t)E;
    p.meta = w.take<int>(p.meta_ints);
    p.rec = w.take<double>((size_t)PG_REC * E);
    p.cbuf = w.take<double>((size_t)E);
    p.Xc = w.take<double>((size_t)16 * N);
    p.H = w.take<double>((size_t)G * dm * dm);
    p.L = w.take<double>((size_t)G * dm * dm);
    p.vec = w.take<double>((size_t)G * 3 * dm);
    return p;
}

extern "C" size_t buf_pose_graph_ws_bytes(int ngraphs, int nodes_total, int edges_total, int max_nodes)
{
    if (ngraphs <= 0 || nodes_total < 0 || edges_total < 0 || max_nodes < 0 || max_nodes > BUF_PG_MAX_NODES) return 0;
    WsCarver w(nullptr, 0);
    carve_pose_graph(w, ngraphs, nodes_total, edges_total, max_nodes);
    return w.used();
}

static bool pg_pos_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

extern "C" int buf_pose_graph_optimize(const int* nodes_host, const int* edges_host, int ngraphs, const int* edge_i_host,
                                       const int* edge_j_host, const double* Z_f64, const double* info_f64,
                                       const unsigned char* uncertain_host, const int* fixed_host, const double* mu_host,
                                       const double* X_init_f64, int max_iterations, double eps_step, double eps_cost, double tau0,
                                       double* X_out_f64, int* status_out, double* cost_out, double* edge_out, void* ws, size_t ws_bytes,
                                       void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    BUF_REQUIRE(ngraphs >= 0, BUF_EINVAL, "buf_pose_graph_optimize: ngraphs=%d", ngraphs);
    BUF_REQUIRE(max_iterations >= 0, BUF_EINVAL, "buf_pose_graph_optimize: max_iterations=%d", max_iterations);
    BUF_REQUIRE(pg_pos_finite(eps_step) && pg_pos_finite(eps_cost) && pg_pos_finite(tau0), BUF_EINVAL,
                "buf_pose_graph_optimize: eps_step=%g eps_cost=%g tau0=%g (each must be finite and > 0)", eps_step, eps_cost, tau0);
    if (ngraphs == 0) return BUF_OK;
    BUF_REQUIRE(nodes_host && edges_host && fixed_host && mu_host, BUF_EINVAL, "buf_pose_graph_optimize: null graph description");
    long long N = 0, E = 0;
    int max_nodes = 0;
    for (int g = 0; g < ngraphs; g++) {
        BUF_REQUIRE(nodes_host[g] >= 0 && edges_host[g] >= 0, BUF_EINVAL, "buf_pose_graph_optimize: graph %d has %d nodes, %d edges", g,
                    nodes_host[g], edges_host[g]);
        BUF_REQUIRE(mu_host[g] >= 0.0 && mu_host[g] <= 1.7976931348623157e308, BUF_EINVAL,
                    "buf_pose_graph_optimize: mu=%g of graph %d (must be finite and >= 0)", mu_host[g], g);
        BUF_REQUIRE(nodes_host[g] == 0 || (fixed_host[g] >= 0 && fixed_host[g] < nodes_host[g]), BUF_EINVAL,
                    "buf_pose_graph_optimize: fixed node %d of graph %d is outside [0, %d)", fixed_host[g], g, nodes_host[g]);
        N += nodes_host[g];
        E += edges_host[g];
        max_nodes = nodes_host[g] > max_nodes ? nodes_host[g] : max_nodes;
    }
    BUF_REQUIRE(N < 0x7fffffffLL / 16 && E < 0x7fffffffLL / PG_REC, BUF_EINVAL, "buf_pose_graph_optimize: %lld nodes, %lld edges (int32 indices)", N, E);
    BUF_REQUIRE(E == 0 || (edge_i_host && edge_j_host && uncertain_host), BUF_EINVAL, "buf_pose_graph_optimize: null edge list");
    {
        long long e = 0;
        for (int g = 0; g < ngraphs; g++)
            for (int k = 0; k < edges_host[g]; k++, e++) {
                const int i = edge_i_host[e], j = edge_j_host[e];
                BUF_REQUIRE(i >= 0 && i < nodes_host[g] && j >= 0 && j < nodes_host[g], BUF_EINVAL,
                            "buf_pose_graph_optimize: edge %d of graph %d names nodes (%d, %d), outside [0, %d)", k, g, i, j, nodes_host[g]);
                BUF_REQUIRE(i != j, BUF_EINVAL, "buf_pose_graph_optimize: edge %d of graph %d joins node %d to itself", k, g, i);
            }
    }
    BUF_REQUIRE(E == 0 || (Z_f64 && info_f64 && edge_out), BUF_EINVAL, "buf_pose_graph_optimize: null edge data or edge output");
    BUF_REQUIRE(N == 0 || (X_init_f64 && X_out_f64), BUF_EINVAL, "buf_pose_graph_optimize: null poses");
    BUF_REQUIRE(status_out && cost_out && ws, BUF_EINVAL, "buf_pose_graph_optimize: null output or workspace");
    BUF_REQUIRE(max_nodes <= BUF_PG_MAX_NODES, BUF_ECAPACITY, "buf_pose_graph_optimize: a graph of %d nodes (capacity %d)", max_nodes,
                BUF_PG_MAX_NODES);
    const size_t need = buf_pose_graph_ws_bytes(ngraphs, (int)N, (int)E, max_nodes);
    BUF_REQUIRE(ws_bytes >= need, BUF_EWORKSPACE, "buf_pose_graph_optimize: workspace %zu < %zu bytes", ws_bytes, need);

    WsCarver w(ws, ws_bytes);
    const PgWs p = carve_pose_graph(w, ngraphs, (int)N, (int)E, max_nodes);
    int* meta = (int*)malloc(sizeof(int) * p.meta_ints);
    BUF_REQUIRE(meta, BUF_EINVAL, "buf_pose_graph_optimize: out of host memory");
    const size_t G = (size_t)ngraphs;
    int* node_off = meta + 2 * G, *edge_off = node_off + G + 1, *fixed = edge_off + G + 1, *ei = fixed + G, *ej = ei + E, *unc = ej + E;
    int* adj_ptr = unc + E, *adj = adj_ptr + N + G;
    memcpy(meta, mu_host, sizeof(double) * G);
    node_off[0] = 0; edge_off[0] = 0;
    for (size_t g = 0; g < G; g++) {
        node_off[g + 1] = node_off[g] + nodes_host[g];
        edge_off[g + 1] = edge_off[g] + edges_host[g];
        fixed[g] = fixed_host[g];
    }
    for (long long e = 0; e < E; e++) { ei[e] = edge_i_host[e]; ej[e] = edge_j_host[e]; unc[e] = uncertain_host[e] ? 1 : 0; }
    for (size_t g = 0; g < G; g++) {                                // per-node adjacency, ascending edge order: (edge << 1) | side
        const int n = nodes_host[g], ne = edges_host[g], e0 = edge_off[g];
        int* ptr = adj_ptr + node_off[g] + g;
        int* lst = adj + 2 * (size_t)e0;
        for (int k = 0; k <= n; k++) ptr[k] = 0;
        for (int e = 0; e < ne; e++) { ptr[ei[e0 + e] + 1]++; ptr[ej[e0 + e] + 1]++; }
        for (int k = 0; k < n; k++) ptr[k + 1] += ptr[k];
        int* fill = (int*)malloc(sizeof(int) * (size_t)(n + 1));
        if (!fill) { free(meta); buf_set_error("buf_pose_graph_optimize: out of host memory"); return BUF_EINVAL; }
        for (int k = 0; k < n; k++) fill[k] = ptr[k];
        for (int e = 0; e < ne; e++) {
            lst[fill[ei[e0 + e]]++] = (e << 1);
            lst[fill[ej[e0 + e]]++] = (e << 1) | 1;
        }
        free(fill);
    }
    int rc = upload_ints(p.meta, meta, (long long)p.meta_ints, "buf_pose_graph_optimize", s);
    free(meta);
    if (rc) return rc;
    PgArgs a;
    a.mu = (const double*)p.meta;
    a.node_off = p.meta + 2 * G; a.edge_off = a.node_off + G + 1; a.fixed = a.edge_off + G + 1;
    a.edge_i = a.fixed + G; a.edge_j = a.edge_i + E; a.unc = a.edge_j + E; a.adj_ptr = a.unc + E; a.adj = a.adj_ptr + N + G;
    a.Z = Z_f64; a.info = info_f64; a.X0 = X_init_f64;
    a.X = X_out_f64; a.status = status_out; a.cost = cost_out; a.edge_out = edge_out;
    a.rec = p.rec; a.cbuf = p.cbuf; a.Xc = p.Xc; a.H = p.H; a.L = p.L; a.vec = p.vec; a.ticks = p.ticks;
    a.max_nodes = max_nodes; a.max_iter = max_iterations;
    a.eps_step = eps_step; a.eps_cost = eps_cost; a.tau0 = tau0;
    k_pose_graph<<<ngraphs, PG_THREADS, 0, s>>>(a);
    BUF_LAUNCH_CHECK();
    return BUF_OK;
}
