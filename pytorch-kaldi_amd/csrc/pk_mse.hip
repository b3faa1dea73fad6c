// pk_mse.hip - the `mse` line of the [model] language (utils.py:2289-2291, :2415-2417) as a fused cost
// (include/pk_amd.h: pk_mse_partial_floats, pk_mse_fwd, pk_mse_bwd).
//
//     loss = (1 / (rows*F)) * sum (a - b)^2          da = (2 / (rows*F)) * dloss * (a - b)          db = -da
//
// a and b are logical [rows][F] fp32 matrices whose last dimension has unit stride and whose rows are lda / ldb floats
// apart: the second operand of the recipes is a column slice of the chunk tensor and is read where it lies.  fp32 in every
// PK_PRECISION mode - it is a cost.  The gradients are written dense, [rows][F].
//
// Three forms, chosen on the host (mse_plan):
//   flat      lda == ldb == F (or a single row) and every pointer 16-byte aligned: the operands are one run of rows*F floats.
//             16-byte loads in a grid-stride loop, four in flight per operand and thread, and a tail of rows*F % 4 floats.
//   quads     the rows of a and b have the SAME misalignment in every row (equal address phase, lda == ldb mod 4), which may
//             still change from row to row: a row is a head of (4 - phase) % 4 floats, aligned 16-byte quads, and a tail.
//             A unit is the head, one quad or the tail; a row has P = ceil(F/4) + 1 units (the last ones may be empty).
//   scalar    anything else - a slice at an odd column of the chunk against a dense module output: a unit is one float.
//   In the last two the units of all rows form ONE sequence, row-major, that is cut into equal runs, one per workgroup;
//   thread t of a workgroup takes units t, t + 256, ... of its run and carries (row, unit in row) along with two adds and a
//   compare, so consecutive lanes read consecutive columns, a wave covers several rows when a row has fewer than 64 units
//   and a long row is split over lanes and workgroups.
//
// Forward reduction, the same bits on every run: per-thread fp32 sums, a butterfly over the wave, four wave sums through
// LDS, ONE partial per workgroup, and mse_finish_kernel (one wave) that adds the partials in a fixed order in double and
// writes the fp32 loss.  No atomics.  A problem that one workgroup covers (rows*F <= MSE_WG_FLOATS) writes the loss itself:
// one launch.  NaN / Inf propagate: nothing here compares or clamps.
//
// Backward is one launch in the same three forms; dloss is read from device memory (no host sync, graph safe), a and b are
// read again rather than a saved difference (the same traffic, nothing kept alive between the passes).
#include <algorithm>

#include "pk_common.h"

namespace {

constexpr int MSE_THREADS = 256;
constexpr long MSE_WG_FLOATS = 8192;  // forward: a workgroup is given at least this many elements (32 per thread)
constexpr long MSE_BWD_FLOATS = 4096;  // backward: no reduction to amortise, and the stores want more waves in flight
constexpr int MSE_WG_PER_CU = 4;
constexpr int MSE_MAX_WGS = 2048;  // caps the partial buffer at 8 KB
enum { MSE_FLAT = 0, MSE_QUADS = 1, MSE_SCALAR = 2 };

struct MsePlan {
    int form, grid, P, phase;  // P: units per row; phase: (address / 4) % 4 of row 0, common to a and b (quads)
    long rows, n, lda, ldb, units, run;
    int F;
};

__device__ __forceinline__ float mse_sq4(f32x4 x, f32x4 y, float acc) {
    const f32x4 d = x - y;
    acc = fmaf(d[0], d[0], acc);
    acc = fmaf(d[1], d[1], acc);
    acc = fmaf(d[2], d[2], acc);
    return fmaf(d[3], d[3], acc);
}

// the workgroup's sum -> partial[blockIdx.x], or the finished loss when this workgroup is the whole grid
__device__ __forceinline__ void mse_block_sum(float v, long n, float* __restrict__ partial, float* __restrict__ loss) {
    __shared__ float sh[MSE_THREADS / PK_WAVE];
    v = pk_wave_sum(v);
    if ((threadIdx.x & (PK_WAVE - 1)) == 0) sh[threadIdx.x / PK_WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (loss) *loss = (float)((double)s / (double)n);
        else partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(MSE_THREADS) void mse_fwd_flat_kernel(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                                   float* __restrict__ partial, float* __restrict__ loss) {
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
    const long n4 = n >> 2, stride = (long)gridDim.x * MSE_THREADS;
    long i = (long)blockIdx.x * MSE_THREADS + threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 x0 = a4[i], x1 = a4[i + stride], x2 = a4[i + 2 * stride], x3 = a4[i + 3 * stride];
        const f32x4 y0 = b4[i], y1 = b4[i + stride], y2 = b4[i + 2 * stride], y3 = b4[i + 3 * stride];
        s0 = mse_sq4(x0, y0, s0);
        s1 = mse_sq4(x1, y1, s1);
        s2 = mse_sq4(x2, y2, s2);
        s3 = mse_sq4(x3, y3, s3);
    }
    for (; i < n4; i += stride) s0 = mse_sq4(a4[i], b4[i], s0);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float d = a[4 * n4 + threadIdx.x] - b[4 * n4 + threadIdx.x];
        s1 = fmaf(d, d, s1);
    }
    mse_block_sum((s0 + s1) + (s2 + s3), n, partial, loss);
}

__global__ __launch_bounds__(PK_WAVE) void mse_finish_kernel(const float* __restrict__ partial, int count, long n,
                                                             float* __restrict__ loss) {
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += PK_WAVE) s += (double)partial[i];
#pragma unroll
    for (int o = PK_WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, PK_WAVE);
    if (threadIdx.x == 0) *loss = (float)(s / (double)n);
}

// ---- the pitched forms ----------------------------------------------------------------------------------------------
// Columns [c0, c1) of row r that unit u covers, and whether they are one aligned quad.
__device__ __forceinline__ bool mse_quad_unit(const MsePlan& g, long r, int u, int& c0, int& c1) {
    const int head = min((4 - (int)((g.phase + r * g.lda) & 3)) & 3, g.F);
    if (u == 0) {
        c0 = 0, c1 = head;
        return false;
    }
    c0 = head + 4 * (u - 1);
    c1 = min(c0 + 4, g.F);
    return c0 + 4 <= g.F;
}

// Walks the units of this thread: f(r, u) for each.  (r, u) advance by MSE_THREADS units without a division.
template <class Fn>
__device__ __forceinline__ void mse_walk(const MsePlan& g, Fn f) {
    long i = (long)blockIdx.x * g.run + threadIdx.x;
    const long last = (long)(blockIdx.x + 1) * g.run, end = last < g.units ? last : g.units;
    if (i >= end) return;
    long r = i / g.P;
    int u = (int)(i - r * g.P);
    const int dr = MSE_THREADS / g.P, du = MSE_THREADS % g.P;
#pragma unroll 4
    for (; i < end; i += MSE_THREADS) {
        f(r, u);
        u += du, r += dr;
        if (u >= g.P) u -= g.P, ++r;
    }
}

template <bool QUADS>
__global__ __launch_bounds__(MSE_THREADS) void mse_fwd_pitched_kernel(MsePlan g, const float* __restrict__ a, const float* __restrict__ b,
                                                                      float* __restrict__ partial, float* __restrict__ loss) {
    float acc = 0.f;
    mse_walk(g, [&](long r, int u) {
        const float* ar = a + r * g.lda;
        const float* br = b + r * g.ldb;
        if (!QUADS) {
            const float d = ar[u] - br[u];
            acc = fmaf(d, d, acc);
            return;
        }
        int c0, c1;
        if (mse_quad_unit(g, r, u, c0, c1)) {
            acc = mse_sq4(*reinterpret_cast<const f32x4*>(ar + c0), *reinterpret_cast<const f32x4*>(br + c0), acc);
        } else {
            for (int c = c0; c < c1; ++c) {
                const float d = ar[c] - br[c];
                acc = fmaf(d, d, acc);
            }
        }
    });
    mse_block_sum(acc, g.n, partial, loss);
}

__device__ __forceinline__ bool mse_aligned16(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(MSE_THREADS) void mse_bwd_flat_kernel(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                                   const float* __restrict__ dloss, float* __restrict__ da,
                                                                   float* __restrict__ db) {
    const float s = (float)(2.0 / (double)n) * dloss[0];
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
    const long n4 = n >> 2, stride = (long)gridDim.x * MSE_THREADS;
    for (long i = (long)blockIdx.x * MSE_THREADS + threadIdx.x; i < n4; i += stride) {
        const f32x4 g = (a4[i] - b4[i]) * s;
        if (da) reinterpret_cast<f32x4*>(da)[i] = g;
        if (db) reinterpret_cast<f32x4*>(db)[i] = -g;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = 4 * n4 + threadIdx.x;
        const float g = (a[i] - b[i]) * s;
        if (da) da[i] = g;
        if (db) db[i] = -g;
    }
}

template <bool QUADS>
__global__ __launch_bounds__(MSE_THREADS) void mse_bwd_pitched_kernel(MsePlan g, const float* __restrict__ a, const float* __restrict__ b,
                                                                      const float* __restrict__ dloss, float* __restrict__ da,
                                                                      float* __restrict__ db) {
    const float s = (float)(2.0 / (double)g.n) * dloss[0];
    mse_walk(g, [&](long r, int u) {
        const float* ar = a + r * g.lda;
        const float* br = b + r * g.ldb;
        const long o = r * g.F;  // the gradients are dense
        int c0 = u, c1 = u + 1;
        if (QUADS && mse_quad_unit(g, r, u, c0, c1)) {
            const f32x4 v = (*reinterpret_cast<const f32x4*>(ar + c0) - *reinterpret_cast<const f32x4*>(br + c0)) * s;
            // (a dense row starts at r*F floats: its quads are aligned only in the rows whose start shares the operands' phase)
            if (da && mse_aligned16(da + o + c0)) {
                *reinterpret_cast<f32x4*>(da + o + c0) = v;
            } else if (da) {
#pragma unroll
                for (int k = 0; k < 4; ++k) da[o + c0 + k] = v[k];
            }
            if (db && mse_aligned16(db + o + c0)) {
                *reinterpret_cast<f32x4*>(db + o + c0) = -v;
            } else if (db) {
#pragma unroll
                for (int k = 0; k < 4; ++k) db[o + c0 + k] = -v[k];
            }
            return;
        }
        for (int c = c0; c < c1; ++c) {
            const float v = (ar[c] - br[c]) * s;
            if (da) da[o + c] = v;
            if (db) db[o + c] = -v;
        }
    });
}

inline int mse_phase(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }
inline bool mse_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int mse_shape(const char* who, int64_t rows, int64_t F, int64_t lda, int64_t ldb) {
    PK_REQUIRE(rows >= 1 && F >= 1, "%s: rows = %lld, F = %lld (at least 1 each)", who, (long long)rows, (long long)F);
    PK_REQUIRE(F <= (1LL << 30) && rows <= (1LL << 40) / F, "%s: rows = %lld, F = %lld (F <= 2^30, rows*F <= 2^40)", who,
               (long long)rows, (long long)F);
    PK_REQUIRE(lda >= F && ldb >= F, "%s: row pitch below the row length: lda = %lld, ldb = %lld, F = %lld", who, (long long)lda,
               (long long)ldb, (long long)F);
    return 0;
}

int mse_grid(long n, long per_wg) {
    const long cap = std::min((long)MSE_MAX_WGS, (long)MSE_WG_PER_CU * pk_num_cu());
    return (int)std::max(1L, std::min(cap, (n + per_wg - 1) / per_wg));
}

// flat_ok: every pointer the flat form would touch is 16-byte aligned
MsePlan mse_plan(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int64_t F, bool flat_ok, long per_wg) {
    MsePlan g;
    g.rows = rows, g.F = (int)F, g.n = rows * F, g.lda = lda, g.ldb = ldb;
    g.grid = mse_grid(g.n, per_wg);
    g.phase = mse_phase(a);
    if ((rows == 1 || (lda == F && ldb == F)) && flat_ok) {
        g.form = MSE_FLAT, g.P = 1, g.units = g.n;
    } else if (F >= 4 && g.phase == mse_phase(b) && (rows == 1 || ((lda - ldb) & 3) == 0)) {
        g.form = MSE_QUADS, g.P = (int)((F + 3) / 4 + 1), g.units = rows * g.P;
    } else {
        g.form = MSE_SCALAR, g.P = (int)F, g.units = g.n;
    }
    g.run = (g.units + g.grid - 1) / g.grid;
    return g;
}

}  // namespace

extern "C" int64_t pk_mse_partial_floats(int64_t rows, int64_t F) {
    if (mse_shape("pk_mse_partial_floats", rows, F, F, F)) return 0;
    return mse_grid(rows * F, MSE_WG_FLOATS);
}

extern "C" int pk_mse_fwd(void* stream, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int64_t F,
                          float* partial, float* loss) {
    if (int rc = mse_shape("pk_mse_fwd", rows, F, lda, ldb)) return rc;
    PK_REQUIRE(a && b && partial && loss, "pk_mse_fwd: a, b, partial or loss are NULL");
    const MsePlan g = mse_plan(a, lda, b, ldb, rows, F, mse_al16(a) && mse_al16(b), MSE_WG_FLOATS);
    float* direct = g.grid == 1 ? loss : nullptr;
    const dim3 grid(g.grid), block(MSE_THREADS);
    if (g.form == MSE_FLAT) {
        hipLaunchKernelGGL(mse_fwd_flat_kernel, grid, block, 0, pk_stream(stream), a, b, g.n, partial, direct);
    } else if (g.form == MSE_QUADS) {
        hipLaunchKernelGGL(mse_fwd_pitched_kernel<true>, grid, block, 0, pk_stream(stream), g, a, b, partial, direct);
    } else {
        hipLaunchKernelGGL(mse_fwd_pitched_kernel<false>, grid, block, 0, pk_stream(stream), g, a, b, partial, direct);
    }
    PK_LAUNCH_CHECK();
    if (g.grid > 1) {
        hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(PK_WAVE), 0, pk_stream(stream), (const float*)partial, g.grid, g.n, loss);
        PK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int pk_mse_bwd(void* stream, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int64_t F,
                          const float* dloss, float* da, float* db) {
    if (int rc = mse_shape("pk_mse_bwd", rows, F, lda, ldb)) return rc;
    PK_REQUIRE(a && b && dloss, "pk_mse_bwd: a, b or dloss are NULL");
    if (!da && !db) return 0;
    const MsePlan g = mse_plan(a, lda, b, ldb, rows, F, mse_al16(a) && mse_al16(b) && mse_al16(da) && mse_al16(db), MSE_BWD_FLOATS);
    const dim3 grid(g.grid), block(MSE_THREADS);
    if (g.form == MSE_FLAT) {
        hipLaunchKernelGGL(mse_bwd_flat_kernel, grid, block, 0, pk_stream(stream), a, b, g.n, dloss, da, db);
    } else if (g.form == MSE_QUADS) {
        hipLaunchKernelGGL(mse_bwd_pitched_kernel<true>, grid, block, 0, pk_stream(stream), g, a, b, dloss, da, db);
    } else {
        hipLaunchKernelGGL(mse_bwd_pitched_kernel<false>, grid, block, 0, pk_stream(stream), g, a, b, dloss, da, db);
    }
    PK_LAUNCH_CHECK();
    return 0;
}
