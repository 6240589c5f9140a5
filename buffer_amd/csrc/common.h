// Shared host/device helpers for libbuffer_hip.so (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/buffer_hip.h"

#define WAVE 64

void buf_set_error(const char* fmt, ...);

#define BUF_CHECK_HIP(expr)                                                            \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            buf_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return BUF_EHIP;                                                           \
        }                                                                              \
    } while (0)

#define BUF_REQUIRE(cond, code, ...)                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            buf_set_error(__VA_ARGS__);                                                \
            return (code);                                                             \
        }                                                                              \
    } while (0)

#define BUF_LAUNCH_CHECK() BUF_CHECK_HIP(hipGetLastError())

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Bump allocator over a caller-provided device workspace.
struct WsCarver {
    char* base;
    size_t off, cap;
    bool ok;
    WsCarver(void* p, size_t bytes) : base((char*)p), off(0), cap(bytes), ok(true) {}
    template <typename T> T* take(size_t count)
    {
        off = align_up(off, 256);
        size_t bytes = count * sizeof(T);
        if (base && off + bytes > cap) ok = false;
        T* r = base ? (T*)(base + off) : nullptr;
        off += bytes;
        return r;
    }
    size_t used() const { return align_up(off, 256); }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device only: the grant is remembered per
// (kernel, device), so a process that drives several GPUs raises the limit on each of them.
#define BUF_MAX_DEVICES 64
struct LdsGrant { size_t bytes[BUF_MAX_DEVICES]; };
int grant_dynamic_lds(const void* kernel, size_t bytes, LdsGrant& g);

// In-place exclusive scan of int32 data[n] on `stream`; tmp must hold scan_tmp_ints() ints.
size_t scan_tmp_ints();
int exclusive_scan_i32(int* data, long long n, int* tmp, int* total_out, hipStream_t stream);

// ---- device helpers ---------------------------------------------------------------------
// Hand-over of LDS data between the lanes of ONE wavefront: the scheduling barrier alone is no memory fence for the compiler
// (IntrNoMem), so it is paired with wavefront-scope release / acquire fences (no instructions on a single wave).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Reference distance: result = 0; result += dx*dx; += dy*dy; += dz*dz  (nanoflann.hpp:433-441).
// __fmul_rn/__fadd_rn are never contracted into FMA.
__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz)
{
    float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    float r = __fmul_rn(dx, dx);
    r = __fadd_rn(r, __fmul_rn(dy, dy));
    r = __fadd_rn(r, __fmul_rn(dz, dz));
    return r;
}

// XCD-aware block order (speed only; MI355X_MICROARCH "Workgroup dispatch": blocks b and b + 8 share an XCD and its L2).
// Logical block of physical block `bid`: the blocks of one XCD take a CONTIGUOUS range of logical blocks, so neighbouring
// work items -- which gather from the same rows -- meet in one L2 instead of being dealt over all eight.  A bijection on [0, nb).
__device__ __forceinline__ int xcd_contiguous_block(int bid, int nb)
{
    const int x = bid & 7, idx = bid >> 3, q = nb >> 3, r = nb & 7;
    return x * q + min(x, r) + idx;
}

// ---- A2 cell-grid lookups (the grid of radius.hip; every kernel that reads it finds a query's cells with these two) ----
// Cell edge and table dims of one element: ext[] = extent of its box (finite, >= 0), cells = slots of its dense table (>= 1).  The
// edge starts strictly larger than the radius (so that |dx| < r never spans two cells + 1) and is coarsened by 1.25 UNTIL the table
// fits: the loop ends by construction, since an edge above the largest extent gives floor(ext / edge) = 0 on every axis, a table of
// one cell (an edge that overflows to +inf included: ext / inf = 0).  dim[] is therefore always taken from a fitting table, every
// dim lies in [1, cells] and the int conversion is exact.  (The loop used to give up after 200 steps -- an extent above
// ~2.4e19 * cells^(1/3) radii, e.g. a 1e30 sentinel point in a cloud searched at 0.07 -- and dim[] then came from a table that did
// not fit, past the int range.)  Host and device run the same fp64 operations in the same order: same edge and dims, bit for bit.
__host__ __device__ inline void grid_cell_dims(const double ext[3], double radius, long long cells, double& edge, int dim[3])
{
    const double fit = cells > 1 ? (double)cells : 1.0;
    double cell = radius > 0 ? radius * 1.00001 : 1.0;
    double d[3];
    for (;;) {
        double tot = 1.0;
        for (int c = 0; c < 3; c++) { d[c] = floor(ext[c] / cell) + 1.0; tot *= d[c]; }
        if (tot <= fit) break;
        cell *= 1.25;
    }
    for (int c = 0; c < 3; c++) dim[c] = (int)d[c];
    edge = cell;
}

// Cell coordinate of a query coordinate v along one axis of an element's grid.  fp64: a query must land in exactly the cell its
// coordinate rounds to (the cell edge exceeds the radius by 1e-5 only).  Clamped to [-2, dim + 1] before the int conversion:
// far-away queries simply find no cell.  (The build side clamps to [0, dim - 1] instead: cell_coord in radius.hip.)
__device__ __forceinline__ int query_cell_coord(float v, float mn, double inv_cell, int dim)
{
    double f = floor(((double)v - (double)mn) * inv_cell);
    f = fmin(fmax(f, -2.0), (double)dim + 1.0);
    return (int)f;
}

// x-run j (0..8: y = cy + j % 3 - 1, z = cz + j / 3 - 1) of the 27-cell block around cell (cx, cy, cz) of an element whose dense
// table starts at table slot toff, dims (dx, dy, dz): rows [start, start + len) of the cell-ordered array (the table holds
// inclusive cell ends).  An empty run (0, 0) where it falls outside the grid, and for j >= 9 (the lanes past the ninth of the
// kernels that fetch one run per lane).  I = the index type of the table offsets.
template <typename I>
__device__ __forceinline__ void cell_xrun(const int* __restrict__ table, I toff, int dx, int dy, int dz, int cx, int cy, int cz, int j,
                                          int& start, int& len)
{
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, dx - 1);
    const int y = cy + (j % 3) - 1, z = cz + (j / 3) - 1;
    start = 0; len = 0;
    if (j < 9 && x0 <= x1 && y >= 0 && y < dy && z >= 0 && z < dz) {
        const I g0 = toff + x0 + (I)dx * (y + (I)dy * z);
        start = g0 == 0 ? 0 : table[g0 - 1];
        len = table[g0 + (x1 - x0)] - start;
    }
}

// element b such that off[b] <= i < off[b+1]
__device__ __forceinline__ int find_elem(const int* __restrict__ off, int nb, int i)
{
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
