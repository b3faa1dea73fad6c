// pk_norm.hip - HBM-bound row/column kernels of the hot path (gfx950):
// BatchNorm statistics / affine+activation+dropout / BatchNorm backward,
// LayerNorm (reference flavour), LogSoftmax, small element-wise helpers.
// All of them stream their operands once with coalesced (column-fastest)
// accesses; reductions are two-stage and deterministic (no atomics).
#include "pk_common.h"

namespace {

constexpr int COLS = 64;   // columns per block (one wave-width, coalesced 256-B rows)
constexpr int RLANES = 4;  // row lanes per block (256 threads)
constexpr int MAX_RB = 256;

__host__ __device__ inline int row_blocks(long M) {
    long rb = (M + 63) / 64;
    if (rb < 1) rb = 1;
    if (rb > MAX_RB) rb = MAX_RB;
    return (int)rb;
}

// ---- BatchNorm statistics: per-column (count, mean, M2), Chan merge ----------
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ x, long ldx, long M, long N,
                                                                float* __restrict__ partial) {
    const int cx = threadIdx.x & (COLS - 1), ry = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * COLS + cx;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per;
    const long r1 = min(M, r0 + rows_per);
    float n = 0.f, shift = 0.f, s = 0.f, ss = 0.f;
    if (c < N) {
        for (long r = r0 + ry; r < r1; r += RLANES) {
            const float v = x[r * ldx + c];
            if (n == 0.f) shift = v;
            const float d = v - shift;
            s += d;
            ss += d * d;
            n += 1.f;
        }
    }
    float mean = 0.f, m2 = 0.f;
    if (n > 0.f) {
        mean = shift + s / n;
        m2 = fmaxf(ss - s * s / n, 0.f);
    }
    __shared__ float sh[RLANES][COLS][3];
    sh[ry][cx][0] = n;
    sh[ry][cx][1] = mean;
    sh[ry][cx][2] = m2;
    __syncthreads();
    if (ry == 0 && c < N) {
        float na = sh[0][cx][0], ma = sh[0][cx][1], qa = sh[0][cx][2];
        for (int k = 1; k < RLANES; ++k) {
            const float nb = sh[k][cx][0], mb = sh[k][cx][1], qb = sh[k][cx][2];
            if (nb > 0.f) {
                const float nt = na + nb, d = mb - ma;
                ma += d * (nb / nt);
                qa += qb + d * d * (na * nb / nt);
                na = nt;
            }
        }
        float* o = partial + ((long)blockIdx.y * N + c) * 3;
        o[0] = na;
        o[1] = ma;
        o[2] = qa;
    }
}

// 16-byte variant: a thread owns 4 consecutive columns (1 KB per wave and row); needs N % 4 == 0, ldx % 4 == 0
// and a 16-byte aligned base.  Same shifted-sum / Chan-merge arithmetic per column as the scalar kernel.
__global__ __launch_bounds__(256) void bn_stats_partial_v4_kernel(const float* __restrict__ x, long ldx, long M, long N,
                                                                   float* __restrict__ partial) {
    const int cx = threadIdx.x & (COLS - 1), ry = threadIdx.x >> 6;
    const long c = ((long)blockIdx.x * COLS + cx) * 4;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per;
    const long r1 = min(M, r0 + rows_per);
    float n = 0.f, shift[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < N) {
#pragma unroll 4
        for (long r = r0 + ry; r < r1; r += RLANES) {
            const float4 v4 = *reinterpret_cast<const float4*>(x + r * ldx + c);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            if (n == 0.f) {
#pragma unroll
                for (int e = 0; e < 4; ++e) shift[e] = v[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[e] - shift[e];
                s[e] += d;
                ss[e] += d * d;
            }
            n += 1.f;
        }
    }
    __shared__ float sh[RLANES][COLS][4][3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float mean = 0.f, m2 = 0.f;
        if (n > 0.f) {
            mean = shift[e] + s[e] / n;
            m2 = fmaxf(ss[e] - s[e] * s[e] / n, 0.f);
        }
        sh[ry][cx][e][0] = n;
        sh[ry][cx][e][1] = mean;
        sh[ry][cx][e][2] = m2;
    }
    __syncthreads();
    // 256 threads: (column group 0..63, element 0..3)
    const int oc = threadIdx.x >> 2, oe = threadIdx.x & 3;
    const long ocol = ((long)blockIdx.x * COLS + oc) * 4 + oe;
    if (ocol < N) {
        float na = sh[0][oc][oe][0], ma = sh[0][oc][oe][1], qa = sh[0][oc][oe][2];
        for (int k = 1; k < RLANES; ++k) {
            const float nb = sh[k][oc][oe][0], mb = sh[k][oc][oe][1], qb = sh[k][oc][oe][2];
            if (nb > 0.f) {
                const float nt = na + nb, d = mb - ma;
                ma += d * (nb / nt);
                qa += qb + d * d * (na * nb / nt);
                na = nt;
            }
        }
        float* o = partial + ((long)blockIdx.y * N + ocol) * 3;
        o[0] = na;
        o[1] = ma;
        o[2] = qa;
    }
}

// Final merges: a block is 32 columns x 8 row-groups.  Group q folds partial rows q, q+8, ... (their loads are
// independent of the running merge, so four are kept in flight), then thread (c, 0) folds the eight group results in
// order - a fixed reduction tree, deterministic run to run.
constexpr int FIN_COLS = 32, FIN_GROUPS = 8;

__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
    if (nb > 0.f) {
        const float nt = na + nb, d = mb - ma;
        ma += d * (nb / nt);
        qa += qb + d * d * (na * nb / nt);
        na = nt;
    }
}

__global__ __launch_bounds__(FIN_COLS* FIN_GROUPS) void bn_stats_final_kernel(const float* __restrict__ partial, int rb, long N,
                                                                             float* __restrict__ mean,
                                                                             float* __restrict__ var) {
    __shared__ float sh[FIN_GROUPS][FIN_COLS][3];
    const int cx = threadIdx.x & (FIN_COLS - 1), q = threadIdx.x / FIN_COLS;
    const long c = (long)blockIdx.x * FIN_COLS + cx;
    float na = 0.f, ma = 0.f, qa = 0.f;
    if (c < N) {
        int k = q;
        for (; k + 3 * FIN_GROUPS < rb; k += 4 * FIN_GROUPS) {
            float v[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* o = partial + ((long)(k + u * FIN_GROUPS) * N + c) * 3;
                v[u][0] = o[0], v[u][1] = o[1], v[u][2] = o[2];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) chan_merge(na, ma, qa, v[u][0], v[u][1], v[u][2]);
        }
        for (; k < rb; k += FIN_GROUPS) {
            const float* o = partial + ((long)k * N + c) * 3;
            chan_merge(na, ma, qa, o[0], o[1], o[2]);
        }
    }
    sh[q][cx][0] = na, sh[q][cx][1] = ma, sh[q][cx][2] = qa;
    __syncthreads();
    if (q == 0 && c < N) {
        for (int g = 1; g < FIN_GROUPS; ++g) chan_merge(na, ma, qa, sh[g][cx][0], sh[g][cx][1], sh[g][cx][2]);
        mean[c] = ma;
        var[c] = na > 0.f ? qa / na : 0.f;  // biased, as BatchNorm normalises with
    }
}

__global__ void bn_finalize_kernel(long N, const float* __restrict__ mean, const float* __restrict__ var,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                   float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ rmean,
                                   float* __restrict__ rvar, float momentum, float unbias) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const float m = mean[c], v = var[c];
    const float inv = 1.0f / sqrtf(v + eps);
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float sc = g * inv;
    scale[c] = sc;
    shift[c] = b - m * sc;
    if (rmean) {
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * m;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (v * unbias);
    }
}

// The same for the concatenated gates of a recurrent layer, whose running statistics live in one BatchNorm1d module
// per gate (neural_networks.py:1052-1055: bn_wh, bn_wz, ...): gate g owns columns [g*H, (g+1)*H).
struct BnGateBufs {
    float* rmean[4];
    float* rvar[4];
    long long* batches[4];
};
__global__ void bn_finalize_gates_kernel(int G, int H, const float* __restrict__ mean, const float* __restrict__ var,
                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                         float* __restrict__ scale, float* __restrict__ shift, BnGateBufs bufs,
                                         float momentum, float unbias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= G * H) return;
    const int g = c / H, j = c - g * H;
    const float m = mean[c], v = var[c];
    const float inv = 1.0f / sqrtf(v + eps);
    const float ga = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float sc = ga * inv;
    scale[c] = sc;
    shift[c] = b - m * sc;
    float* rm = bufs.rmean[g];
    float* rv = bufs.rvar[g];
    rm[j] = (1.f - momentum) * rm[j] + momentum * m;
    rv[j] = (1.f - momentum) * rv[j] + momentum * (v * unbias);
    if (j == 0 && bufs.batches[g] != nullptr) bufs.batches[g][0] += 1;  // num_batches_tracked
}

// bn_stats_final_kernel + bn_finalize_gates_kernel in one launch (a recurrent layer's projection in training mode: the
// statistics partials of the GEMM epilogue -> mean / var, scale / shift, running statistics of every gate's module)
__global__ __launch_bounds__(FIN_COLS* FIN_GROUPS) void bn_stats_final_gates_kernel(const float* __restrict__ partial, int rb, int G,
                                                                                   int H, float* __restrict__ mean,
                                                                                   float* __restrict__ var,
                                                                                   const float* __restrict__ gamma,
                                                                                   const float* __restrict__ beta, float eps,
                                                                                   float* __restrict__ scale,
                                                                                   float* __restrict__ shift, BnGateBufs bufs,
                                                                                   float momentum, float unbias) {
    __shared__ float sh[FIN_GROUPS][FIN_COLS][3];
    const long N = (long)G * H;
    const int cx = threadIdx.x & (FIN_COLS - 1), q = threadIdx.x / FIN_COLS;
    const long c = (long)blockIdx.x * FIN_COLS + cx;
    float na = 0.f, ma = 0.f, qa = 0.f;
    if (c < N) {
        int k = q;
        for (; k + 3 * FIN_GROUPS < rb; k += 4 * FIN_GROUPS) {
            float v[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* o = partial + ((long)(k + u * FIN_GROUPS) * N + c) * 3;
                v[u][0] = o[0], v[u][1] = o[1], v[u][2] = o[2];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) chan_merge(na, ma, qa, v[u][0], v[u][1], v[u][2]);
        }
        for (; k < rb; k += FIN_GROUPS) {
            const float* o = partial + ((long)k * N + c) * 3;
            chan_merge(na, ma, qa, o[0], o[1], o[2]);
        }
    }
    sh[q][cx][0] = na, sh[q][cx][1] = ma, sh[q][cx][2] = qa;
    __syncthreads();
    if (q == 0 && c < N) {
        for (int g = 1; g < FIN_GROUPS; ++g) chan_merge(na, ma, qa, sh[g][cx][0], sh[g][cx][1], sh[g][cx][2]);
        const float m = ma, v = na > 0.f ? qa / na : 0.f;  // biased, as BatchNorm normalises with
        mean[c] = m;
        var[c] = v;
        const int g = (int)(c / H), j = (int)(c - (long)g * H);
        const float inv = 1.0f / sqrtf(v + eps);
        const float sc = (gamma ? gamma[c] : 1.f) * inv;
        scale[c] = sc;
        shift[c] = (beta ? beta[c] : 0.f) - m * sc;
        float* rm = bufs.rmean[g];
        float* rv = bufs.rvar[g];
        rm[j] = (1.f - momentum) * rm[j] + momentum * m;
        rv[j] = (1.f - momentum) * rv[j] + momentum * (v * unbias);
        if (j == 0 && bufs.batches[g] != nullptr) bufs.batches[g][0] += 1;  // num_batches_tracked
    }
}

// ---- y = mask * act(x*scale + shift) ----------------------------------------
__global__ void affine_act_fwd_kernel(const float* __restrict__ x, long ldx, long M, long N,
                                      const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                      const float* __restrict__ mask, float* __restrict__ y, long ldy) {
    const long total = M * N;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / N, c = i - r * N;
        float v = x[r * ldx + c];
        if (scale) v = v * scale[c] + shift[c];
        v = pk_act(act, v);
        if (mask) v *= mask[i];
        y[r * ldy + c] = v;
    }
}

__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                               const float* __restrict__ mask, int act, long n, float* __restrict__ g) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = dy[i];
        if (mask) v *= mask[i];
        // `a` is the activation output BEFORE dropout when mask is given
        g[i] = v * pk_act_grad_from_out(act, a[i]);
    }
}

// The element arithmetic of the exact-fp32 BatchNorm-backward passes, shared by their scalar and 16-byte forms with the
// contraction spelled out: the compiler contracts a loop-invariant product differently in the two loop shapes, and aligned
// and unaligned operands must not give different bits.  The forms chosen are the ones the scalar kernels had compiled to since
// round 1 (the 30-step trajectory fixture is pinned on those bits: any other rounding of these two lines moves it past 1e-4).
__device__ __forceinline__ float bnb_f32_xhat(float x, float mu, float inv) {
#pragma clang fp contract(off)
    return (x - mu) * inv;
}
__device__ __forceinline__ float bnb_f32_gx(float gv, float xh, float acc) {  // acc + round(gv * xh): no fma
#pragma clang fp contract(off)
    const float t = gv * xh;
    return acc + t;
}
__device__ __forceinline__ float bnb_f32_dx(float ga, float inv, float gv, float sg, float sx, float xh, float inv_count) {
#pragma clang fp contract(off)
    const float t0 = __builtin_fmaf(-inv_count, sg, gv);
    const float t1 = (xh * sx) * inv_count;
    return (ga * inv) * (t0 - t1);
}

// ---- BatchNorm backward reductions --------------------------------------------
// MODE 0: sum_g, sum_g*xhat   MODE 1: column sum only
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_partial_kernel(const float* __restrict__ g,
                                                                  const float* __restrict__ g2, long ldg,
                                                                  const float* __restrict__ x, long ldx, long M, long N,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ var, float eps,
                                                                  float* __restrict__ partial) {
    const int cx = threadIdx.x & (COLS - 1), ry = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * COLS + cx;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per;
    const long r1 = min(M, r0 + rows_per);
    float s0 = 0.f, s1 = 0.f;
    if (c < N) {
        float mu = 0.f, inv = 0.f;
        if (MODE == 0) {
            mu = mean[c];
            inv = 1.0f / sqrtf(var[c] + eps);
        }
        for (long r = r0 + ry; r < r1; r += RLANES) {
            float gv = g[r * ldg + c];
            if (g2) gv += g2[r * ldg + c];
            s0 += gv;
            if (MODE == 0) s1 = bnb_f32_gx(gv, bnb_f32_xhat(x[r * ldx + c], mu, inv), s1);
        }
    }
    __shared__ float sh[RLANES][COLS][2];
    sh[ry][cx][0] = s0;
    sh[ry][cx][1] = s1;
    __syncthreads();
    if (ry == 0 && c < N) {
        float a0 = 0.f, a1 = 0.f;
        for (int k = 0; k < RLANES; ++k) {
            a0 += sh[k][cx][0];
            a1 += sh[k][cx][1];
        }
        float* o = partial + ((long)blockIdx.y * N + c) * 2;
        o[0] = a0;
        o[1] = a1;
    }
}

// The same reduction with a thread owning FOUR consecutive columns (16-byte loads; two rows in flight per thread): the
// scalar form above reads 4 bytes per lane and load and runs at 1.7-1.9 TB/s on the exact-fp32 mode's [64000 x 1100..2200]
// gate gradients.  Same row lanes, same rows per lane in the same order, same expression per column: the partial sums are
// bit-identical to the scalar form's (tests/test_gpu_kernels.py::test_bn_bwd_f32_forms_bit_identical).  Needs 16-byte
// aligned operands and N, ldg, ldx multiples of 4.
template <int V> struct BnVec;
template <> struct BnVec<4> { typedef f32x4 T; };
template <> struct BnVec<2> { typedef pk_f32x2 T; };
template <int MODE, int V>  // V = 4 (16-byte) or 2 (8-byte accesses: rows of 1650 floats - the GRU - are 8-byte aligned)
__global__ __launch_bounds__(256) void col_reduce_partial_vec_kernel(const float* __restrict__ g,
                                                                     const float* __restrict__ g2, long ldg,
                                                                     const float* __restrict__ x, long ldx, long M, long N,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ var, float eps,
                                                                     float* __restrict__ partial) {
    typedef typename BnVec<V>::T VT;
    constexpr int VCOLS = 64 * V;  // columns per block
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * VCOLS + cx * V;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per;
    const long r1 = min(M, r0 + rows_per);
    VT s0 = VT(0.f), s1 = VT(0.f);
    if (c < N) {
        VT mu = VT(0.f), inv = VT(0.f);
        if (MODE == 0) {
            mu = *reinterpret_cast<const VT*>(mean + c);
            const VT vv = *reinterpret_cast<const VT*>(var + c);
#pragma unroll
            for (int e = 0; e < V; ++e) inv[e] = 1.0f / sqrtf(vv[e] + eps);
        }
        const VT zero = VT(0.f);
        for (long r = r0 + ry; r < r1; r += 2 * RLANES) {
            const bool second = r + RLANES < r1;
            const long rs = second ? r + RLANES : r;  // (clamped: no branch around a load)
            const VT ga = *reinterpret_cast<const VT*>(g + r * ldg + c);
            const VT gb = *reinterpret_cast<const VT*>(g + rs * ldg + c);
            const VT ha = g2 ? *reinterpret_cast<const VT*>(g2 + r * ldg + c) : zero;
            const VT hb = g2 ? *reinterpret_cast<const VT*>(g2 + rs * ldg + c) : zero;
            VT xa = zero, xb = zero;
            if (MODE == 0) {
                xa = *reinterpret_cast<const VT*>(x + r * ldx + c);
                xb = *reinterpret_cast<const VT*>(x + rs * ldx + c);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float gv = ga[e];
                if (g2) gv += ha[e];
                s0[e] += gv;
                if (MODE == 0) s1[e] = bnb_f32_gx(gv, bnb_f32_xhat(xa[e], mu[e], inv[e]), s1[e]);
            }
            if (second) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float gv = gb[e];
                    if (g2) gv += hb[e];
                    s0[e] += gv;
                    if (MODE == 0) s1[e] = bnb_f32_gx(gv, bnb_f32_xhat(xb[e], mu[e], inv[e]), s1[e]);
                }
            }
        }
    }
    __shared__ float sh[RLANES][VCOLS][2];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        sh[ry][cx * V + e][0] = s0[e];
        sh[ry][cx * V + e][1] = s1[e];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < VCOLS; o += 256) {
        const long cc = (long)blockIdx.x * VCOLS + o;
        if (cc >= N) continue;
        float a0 = 0.f, a1 = 0.f;
        for (int k = 0; k < RLANES; ++k) {
            a0 += sh[k][o][0];
            a1 += sh[k][o][1];
        }
        float* op = partial + ((long)blockIdx.y * N + cc) * 2;
        op[0] = a0;
        op[1] = a1;
    }
}

// Final column sums of [rb][N][2] partials: a block is 16 columns x 16 row-groups (N / 16 blocks: 69 at N = 1100 - with 32
// columns per block the 35 blocks of the first version took 40 us per call, seven calls per training step); a thread
// keeps eight partial rows in flight; fixed reduction order, deterministic run to run.
constexpr int CF_COLS = 16, CF_GROUPS = 16;
// acc0 / acc1 (optional): the sums are also ADDED there (the flat .grad of BatchNorm shift / scale: no add launch behind it).
// pad (optional): the pad columns [pad_n0, pad_pitch) of a bf16 matrix of pad_rows rows are zeroed on the way (the matrix
// the caller's next kernel fills; its own zero-fill launch is gone).
__global__ __launch_bounds__(CF_COLS* CF_GROUPS) void col_reduce_final_kernel(const float* __restrict__ partial, int rb, long N,
                                                                             float* __restrict__ out0,
                                                                             float* __restrict__ out1,
                                                                             float* __restrict__ acc0,
                                                                             float* __restrict__ acc1,
                                                                             unsigned short* __restrict__ pad, long pad_pitch,
                                                                             long pad_rows, int pad_n0) {
    __shared__ float sh[CF_GROUPS][CF_COLS][2];
    const int cx = threadIdx.x & (CF_COLS - 1), q = threadIdx.x / CF_COLS;
    const long c = (long)blockIdx.x * CF_COLS + cx;
    float a0 = 0.f, a1 = 0.f;
    if (c < N) {
        int k = q;
        for (; k + 7 * CF_GROUPS < rb; k += 8 * CF_GROUPS) {
            float2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float2*>(partial + ((long)(k + u * CF_GROUPS) * N + c) * 2);
#pragma unroll
            for (int u = 0; u < 8; ++u) a0 += v[u].x, a1 += v[u].y;
        }
        for (; k < rb; k += CF_GROUPS) {
            const float2 v = *reinterpret_cast<const float2*>(partial + ((long)k * N + c) * 2);
            a0 += v.x, a1 += v.y;
        }
    }
    sh[q][cx][0] = a0, sh[q][cx][1] = a1;
    __syncthreads();
    if (q == 0 && c < N) {
        for (int g = 1; g < CF_GROUPS; ++g) a0 += sh[g][cx][0], a1 += sh[g][cx][1];
        out0[c] = a0;
        if (out1) out1[c] = a1;
        if (acc0) acc0[c] += a0;
        if (acc1) acc1[c] += a1;
    }
    if (pad != nullptr) {
        const int w = (int)pad_pitch - pad_n0;
        const long nt = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
        if ((w & 3) == 0 && (pad_n0 & 3) == 0 && (pad_pitch & 3) == 0 && ((uintptr_t)pad & 7) == 0) {  // 8-byte stores
            const int wq = w >> 2;
            const long total = pad_rows * wq;
            for (long i = t0; i < total; i += nt) {
                const long r = i / wq;
                *reinterpret_cast<uint2*>(pad + r * pad_pitch + pad_n0 + 4 * (i - r * wq)) = make_uint2(0u, 0u);
            }
        } else {
            const long total = pad_rows * w;
            for (long i = t0; i < total; i += nt) {
                const long r = i / w;
                pad[r * pad_pitch + pad_n0 + (i - r * w)] = 0;
            }
        }
    }
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ g2, long ldg,
                                    const float* __restrict__ x, long ldx, long M, long N,
                                    const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                    const float* __restrict__ gamma, const float* __restrict__ sum_g,
                                    const float* __restrict__ sum_gx, float inv_count, float* __restrict__ dx,
                                    long lddx) {
    const long total = M * N;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / N, c = i - r * N;
        const float inv = 1.0f / sqrtf(var[c] + eps);
        const float xh = bnb_f32_xhat(x[r * ldx + c], mean[c], inv);
        float gv = g[r * ldg + c];
        if (g2) gv += g2[r * ldg + c];
        const float ga = gamma ? gamma[c] : 1.f;
        dx[r * lddx + c] = bnb_f32_dx(ga, inv, gv, sum_g[c], sum_gx[c], xh, inv_count);
    }
}

// ... and its 16-byte form (a thread owns four consecutive columns of a strip of rows; the per-column constants are formed
// once per thread instead of one 64-bit division, one square root and five gathers per element): the same expression
// per element, bit-identical results.
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_vec_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                               long ldg, const float* __restrict__ x, long ldx, long M,
                                                               long N, const float* __restrict__ mean,
                                                               const float* __restrict__ var, float eps,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ sum_g,
                                                               const float* __restrict__ sum_gx, float inv_count,
                                                               float* __restrict__ dx, long lddx) {
    typedef typename BnVec<V>::T VT;
    constexpr int VCOLS = 64 * V;
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * VCOLS + cx * V;
    if (c >= N) return;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per;
    const long r1 = min(M, r0 + rows_per);
    const VT mu = *reinterpret_cast<const VT*>(mean + c), vv = *reinterpret_cast<const VT*>(var + c);
    const VT sg = *reinterpret_cast<const VT*>(sum_g + c), sx = *reinterpret_cast<const VT*>(sum_gx + c);
    VT ga = VT(1.f), inv;
    if (gamma) ga = *reinterpret_cast<const VT*>(gamma + c);
#pragma unroll
    for (int e = 0; e < V; ++e) inv[e] = 1.0f / sqrtf(vv[e] + eps);
    const VT zero = VT(0.f);
    for (long r = r0 + ry; r < r1; r += 2 * RLANES) {
        const bool second = r + RLANES < r1;
        const long rs = second ? r + RLANES : r;
        const VT ga_ = *reinterpret_cast<const VT*>(g + r * ldg + c);
        const VT gb_ = *reinterpret_cast<const VT*>(g + rs * ldg + c);
        const VT ha = g2 ? *reinterpret_cast<const VT*>(g2 + r * ldg + c) : zero;
        const VT hb = g2 ? *reinterpret_cast<const VT*>(g2 + rs * ldg + c) : zero;
        const VT xa = *reinterpret_cast<const VT*>(x + r * ldx + c);
        const VT xb = *reinterpret_cast<const VT*>(x + rs * ldx + c);
        VT oa, ob;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float xh = bnb_f32_xhat(xa[e], mu[e], inv[e]);
            float gv = ga_[e];
            if (g2) gv += ha[e];
            oa[e] = bnb_f32_dx(ga[e], inv[e], gv, sg[e], sx[e], xh, inv_count);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float xh = bnb_f32_xhat(xb[e], mu[e], inv[e]);
            float gv = gb_[e];
            if (g2) gv += hb[e];
            ob[e] = bnb_f32_dx(ga[e], inv[e], gv, sg[e], sx[e], xh, inv_count);
        }
        *reinterpret_cast<VT*>(dx + r * lddx + c) = oa;
        if (second) *reinterpret_cast<VT*>(dx + rs * lddx + c) = ob;
    }
}

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ o) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        o[i] = a[i] + b[i];
}

// ---- block reductions -----------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = pk_wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    float t = 0.f;
    const int nw = blockDim.x >> 6;
    for (int k = 0; k < nw; ++k) t += sh[k];
    return t;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = pk_wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    float t = -INFINITY;
    const int nw = blockDim.x >> 6;
    for (int k = 0; k < nw; ++k) t = fmaxf(t, sh[k]);
    return t;
}

// ---- LayerNorm of the reference: gamma*(x-mean)/(std_unbiased+eps)+beta ----------
constexpr float LN_FAR = 64.f;  // |mean| / (std + eps) beyond which layernorm_fwd / _bwd correct the rounding of the mean
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, long rows, long F,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             float* __restrict__ y, float* __restrict__ mean_o,
                                                             float* __restrict__ rinv_o) {
    __shared__ float sh[8];
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* xr = x + r * F;
        float s = 0.f;
        for (long f = threadIdx.x; f < F; f += blockDim.x) s += xr[f];
        const float mu = block_sum(s, sh) / (float)F;
        float q = 0.f;
        for (long f = threadIdx.x; f < F; f += blockDim.x) {
            const float d = xr[f] - mu;
            q += d * d;
        }
        float var = block_sum(q, sh) / (float)(F - 1);
        float rinv = 1.0f / (sqrtf(var) + eps);
        // A row far from zero (|mean| > LN_FAR std): mu is rounded to an ulp of the LEVEL, eps * |mean| / std of the spread
        // (1e3 + N(0,1): 5e-5 of y).  x - mu is exact there, so the mean of the deviations IS that rounding error: take it
        // out (the corrected two-pass form).  A select: every other row keeps dc = 0 and its bits.
        float dc = 0.f;
        if (fabsf(mu) * rinv > LN_FAR) {
            float sd = 0.f;
            for (long f = threadIdx.x; f < F; f += blockDim.x) sd += xr[f] - mu;
            sd = block_sum(sd, sh);
            dc = sd / (float)F;
            var = fmaxf(var - sd * dc / (float)(F - 1), 0.f);
            rinv = 1.0f / (sqrtf(var) + eps);
        }
        for (long f = threadIdx.x; f < F; f += blockDim.x)
            y[r * F + f] = gamma[f] * (((xr[f] - mu) - dc) * rinv) + beta[f];
        if (threadIdx.x == 0) {
            mean_o[r] = mu;
            rinv_o[r] = rinv;
        }
    }
}

// dx_i = rinv*(g_i - mean(g)) - rinv^2 * (sum_j g_j d_j) * d_i / ((F-1) * std),  g = dy*gamma, d = x-mean
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             long rows, long F, const float* __restrict__ gamma,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ rinv_i, float eps,
                                                             float* __restrict__ dx, float* __restrict__ dgx) {
    __shared__ float sh[8];
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float mu = mean[r], rinv = rinv_i[r];
        const float stdv = 1.0f / rinv - eps;
        const bool far = fabsf(mu) * rinv > LN_FAR;  // (see layernorm_fwd_kernel: d = (x - mu) - dc on such a row)
        float sg = 0.f, sgd = 0.f, sd = 0.f;
        for (long f = threadIdx.x; f < F; f += blockDim.x) {
            const float g = dy[r * F + f] * gamma[f];
            sg += g;
            sgd += g * (x[r * F + f] - mu);
            if (far) sd += x[r * F + f] - mu;
        }
        sg = block_sum(sg, sh);
        sgd = block_sum(sgd, sh);
        float dc = 0.f;
        if (far) {
            dc = block_sum(sd, sh) / (float)F;
            sgd -= dc * sg;
        }
        const float mg = sg / (float)F;
        // a row of variance 0: torch's std() backward is 0 where std == 0, so the reference's gradient is the finite
        // rinv * (g - mean(g)); sgd / stdv is 0 / 0 here.  A select: rows with std > 0 keep their bits.
        const float k2 = stdv > 0.f ? rinv * rinv * sgd / ((float)(F - 1) * stdv) : 0.f;
        for (long f = threadIdx.x; f < F; f += blockDim.x) {
            const float d = (x[r * F + f] - mu) - dc;
            const float dyv = dy[r * F + f];
            dx[r * F + f] = rinv * (dyv * gamma[f] - mg) - k2 * d;
            if (dgx) dgx[r * F + f] = dyv * (d * rinv);
        }
    }
}

// ---- a conv layer's tail in one launch: drop(act(LayerNorm(z))) with the CNN / SincNet flavour of the reference's
// LayerNorm (neural_networks.py:1510-1512, 1639-1641 - features [C, L], statistics over the last dim only; then
// :1546-1552, :1655-1661).  z: [B, C, L] as rows r = b * C + c of length L; gamma / beta: [C, L].  One WAVE per row
// (rows are 36 .. 1024 samples long in the shipped recipes): shuffles only, no LDS, no barrier.  The same arithmetic as
// layernorm_fwd_kernel + the broadcast affine + affine_act: two-pass statistics, unbiased std + eps.
//   a = act(gamma[c] * ((z - mean) * rinv) + beta[c]),  y = a * mask  (y == nullptr without a mask)
__global__ __launch_bounds__(256) void ln_last_act_drop_fwd_kernel(const float* __restrict__ z, long rows, int C, int L,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, int act,
                                                                    const float* __restrict__ mask, float* __restrict__ a,
                                                                    float* __restrict__ y, float* __restrict__ mean_o,
                                                                    float* __restrict__ rinv_o) {
    const int lane = threadIdx.x & 63;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
        const float* zr = z + r * L;
        const long po = (long)(r % C) * L;
        float s = 0.f;
        for (int f = lane; f < L; f += 64) s += zr[f];
        const float mu = pk_wave_sum(s) / (float)L;
        float q = 0.f;
        for (int f = lane; f < L; f += 64) {
            const float d = zr[f] - mu;
            q += d * d;
        }
        const float var = pk_wave_sum(q) / (float)(L - 1);
        const float rinv = 1.0f / (sqrtf(var) + eps);
        for (int f = lane; f < L; f += 64) {
            const float u = gamma[po + f] * ((zr[f] - mu) * rinv) + beta[po + f];
            const float av = pk_act(act, u);
            a[r * L + f] = av;
            if (y) y[r * L + f] = av * mask[r * L + f];
        }
        if (lane == 0) {
            mean_o[r] = mu;
            rinv_o[r] = rinv;
        }
    }
}
// backward of the same: g = dy * mask * act'(a) (from the OUTPUT, like pk_act_bwd); LayerNorm backward with the row's
// gamma; the parameter-gradient terms leave as pg[b][0][c][f] = g * xhat, pg[b][1][c][f] = g (one column sum over the
// batch then gives d gamma and d beta: pk_colsum on [B, 2 * C * L]).
__global__ __launch_bounds__(256) void ln_last_act_drop_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                                    const float* __restrict__ a,
                                                                    const float* __restrict__ mask, long rows, int C, int L,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ rinv_i, float eps, int act,
                                                                    float* __restrict__ dz, float* __restrict__ pg) {
    const int lane = threadIdx.x & 63;
    const long CL = (long)C * L;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
        const long c = r % C, b = r / C, po = c * L;
        const float mu = mean[r], rinv = rinv_i[r];
        const float stdv = 1.0f / rinv - eps;
        float sg = 0.f, sgd = 0.f;
        for (int f = lane; f < L; f += 64) {
            float g = dy[r * L + f] * pk_act_grad_from_out(act, a[r * L + f]);
            if (mask) g *= mask[r * L + f];
            const float gg = g * gamma[po + f];
            sg += gg;
            sgd += gg * (z[r * L + f] - mu);
        }
        sg = pk_wave_sum(sg);
        sgd = pk_wave_sum(sgd);
        const float mg = sg / (float)L;
        const float k2 = stdv > 0.f ? rinv * rinv * sgd / ((float)(L - 1) * stdv) : 0.f;  // (std == 0: see layernorm_bwd_kernel)
        float* pgx = pg + b * 2 * CL + po;
        for (int f = lane; f < L; f += 64) {
            float g = dy[r * L + f] * pk_act_grad_from_out(act, a[r * L + f]);
            if (mask) g *= mask[r * L + f];
            const float d = z[r * L + f] - mu;
            dz[r * L + f] = rinv * (g * gamma[po + f] - mg) - k2 * d;
            pgx[f] = g * (d * rinv);
            pgx[CL + f] = g;
        }
    }
}

// ---- LogSoftmax(dim=1) -------------------------------------------------------------
// y = x - (m + log(sum)) rounds the log-sum-exp to an ulp of the row's LEVEL m: logits at 1e4 +- 4 come out 5e-5 off, and
// exp(y) in the backward pass with them.  Rows whose maximum lies beyond LSM_FAR are written as (x - m) - log(sum) (the
// first difference is small and nearly exact).  A select on a row-uniform value: rows of ordinary logits keep their bits
// (the one-ulp difference between the two forms moves a 30-step fp32 training trajectory: tests/test_gpu_reference_pins.py).
constexpr float LSM_FAR = 32.f;
__global__ __launch_bounds__(256) void logsoftmax_fwd_kernel(const float* __restrict__ x, long ldx, long rows, long N,
                                                              float* __restrict__ y) {
    __shared__ float sh[8];
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* xr = x + r * ldx;
        float m = -INFINITY;
        for (long c = threadIdx.x; c < N; c += blockDim.x) m = fmaxf(m, xr[c]);
        m = block_max(m, sh);
        float s = 0.f;
        for (long c = threadIdx.x; c < N; c += blockDim.x) s += expf(xr[c] - m);
        s = block_sum(s, sh);
        const float ls = logf(s), lse = m + ls;
        const bool far = fabsf(m) > LSM_FAR;  // (see LSM_FAR)
        for (long c = threadIdx.x; c < N; c += blockDim.x) y[r * N + c] = far ? (xr[c] - m) - ls : xr[c] - lse;
    }
}

__global__ __launch_bounds__(256) void logsoftmax_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              long rows, long N, float* __restrict__ dx) {
    __shared__ float sh[8];
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        float s = 0.f;
        for (long c = threadIdx.x; c < N; c += blockDim.x) s += dy[r * N + c];
        s = block_sum(s, sh);
        for (long c = threadIdx.x; c < N; c += blockDim.x) dx[r * N + c] = dy[r * N + c] - expf(y[r * N + c]) * s;
    }
}

// Wave-per-row variants for rows of up to 64*NPL columns: the row lives in registers (every element is read from
// HBM once, all loads of a lane in flight together) and the reductions are wave shuffles - no LDS, no barriers.
template <int NPL>
__global__ __launch_bounds__(256) void logsoftmax_fwd_wave_kernel(const float* __restrict__ x, long ldx, long rows, long N,
                                                                   float* __restrict__ y, int* __restrict__ amax) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    for (long r = wid; r < rows; r += nw) {
        const float* xr = x + r * ldx;
        float v[NPL];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            v[i] = c < N ? xr[c] : -INFINITY;
            m = fmaxf(m, v[i]);
        }
        m = pk_wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) sum += expf(v[i] - m);  // exp(-inf) = 0 for the padding lanes
        sum = pk_wave_sum(sum);
        const float ls = logf(sum), lse = m + ls;
        const bool far = fabsf(m) > LSM_FAR;  // (see LSM_FAR)
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            v[i] = far ? (v[i] - m) - ls : v[i] - lse;
            if (c < N) y[r * N + c] = v[i];
        }
        if (amax != nullptr) {
            // the row's arg-max over the values just stored, by the rule of nll_err_partial_kernel (first index on ties; a
            // NaN row: the first column), so that the cost kernel behind this output need not read the row again: the
            // frame-error count of cost_err (utils.py:2363-2367) becomes one compare per row
            float best = -INFINITY;
            long besti = N;
#pragma unroll
            for (int i = 0; i < NPL; ++i) {
                const long c = lane + 64 * i;
                const float u = c < N ? v[i] : -INFINITY;
                if (c < N && (u > best || (u == best && c < besti) || besti == N)) best = u, besti = c;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ob = __shfl_xor(best, off);
                const long oi = __shfl_xor(besti, off);
                if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
            }
            if (lane == 0) amax[r] = (int)besti;
        }
    }
}

template <int NPL>
__global__ __launch_bounds__(256) void logsoftmax_bwd_wave_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                   long rows, long N, float* __restrict__ dx, long lddx) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    for (long r = wid; r < rows; r += nw) {
        float g[NPL], e[NPL];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            g[i] = c < N ? dy[r * N + c] : 0.f;
            e[i] = c < N ? y[r * N + c] : -INFINITY;
            sum += g[i];
        }
        sum = pk_wave_sum(sum);
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            if (c < N) dx[r * lddx + c] = g[i] - expf(e[i]) * sum;
            else if (c < lddx) dx[r * lddx + c] = 0.f;  // (pad columns of a re-pitched gradient)
        }
    }
}

// Backward of (Linear -> LogSoftmax) heads in perf mode: dz = dy - exp(y) * sum(dy) is written ONCE, as the bf16 GEMM
// operand the dX / dW GEMMs read (row pitch ldb, pad columns zero), and its column sums (the bias gradient, taken from
// the fp32 values before rounding) are accumulated in registers over the rows a wave owns: the fp32 dz matrix, its
// conversion pass and the column-sum pass never exist (64 000 x 1938: 2.7 GB of HBM traffic -> 1.25 GB).
// ONEHOT: the incoming gradient is that of NLLLoss(reduction = mean) on this output (utils.py:2361) and is never
// materialised: dy[r][c] = -scale at c = lab[r] and zero elsewhere, scale = dloss / count (both read on the device).
template <int NPL, bool ONEHOT>
__global__ __launch_bounds__(256) void logsoftmax_bwd_bf16_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                   const long* __restrict__ lab,
                                                                   const float* __restrict__ dloss,
                                                                   const float* __restrict__ count, long ignore_index,
                                                                   long rows, long N, unsigned short* __restrict__ dxb,
                                                                   long ldb, long pitch, float* __restrict__ partial) {
    // ldb: columns written per row (N values + zero padding); pitch >= ldb: elements between rows (dxb may be a column
    // slice of a wider buffer: several output layers on one input write ONE concatenated operand for a single dX GEMM)
    __shared__ float sh[3][64 * NPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wid = (long)blockIdx.x * 4 + wave, nw = (long)gridDim.x * 4;
    float scale = 0.f;
    if (ONEHOT) {
        const float cnt = count[0];
        scale = cnt > 0.f ? dloss[0] / cnt : 0.f;
    }
    float acc[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) acc[i] = 0.f;
    for (long r = wid; r < rows; r += nw) {
        float g[NPL], e[NPL];
        float sum = 0.f;
        long lr = -1;
        if (ONEHOT) {
            lr = lab[r];
            if (lr == ignore_index || lr < 0 || lr >= N) lr = -1;  // (an out-of-range label is counted by the forward pass)
            sum = lr >= 0 ? -scale : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            if (ONEHOT) g[i] = c == lr ? -scale : 0.f;
            else g[i] = c < N ? dy[r * N + c] : 0.f;
            e[i] = c < N ? y[r * N + c] : -INFINITY;
            if (!ONEHOT) sum += g[i];
        }
        if (!ONEHOT) sum = pk_wave_sum(sum);
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            const float d = c < N ? g[i] - expf(e[i]) * sum : 0.f;
            acc[i] += d;
            if (c < ldb) dxb[r * pitch + c] = pk_f2bf(d);
        }
    }
    // the four waves' column sums -> one partial row per block (the layout col_reduce_final_kernel reads)
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) sh[wave - 1][lane + 64 * i] = acc[i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            if (c < N) {
                float* o = partial + ((long)blockIdx.x * N + c) * 2;
                o[0] = acc[i] + sh[0][c] + sh[1][c] + sh[2][c];
                o[1] = 0.f;
            }
        }
    }
}

// NLLLoss(reduction = mean, ignore_index) and the frame error rate of the reference's cost_nll / cost_err lines
// (utils.py:2361-2367: loss = NLLLoss()(out, lab); err = mean(argmax(out, 1) != lab)) in ONE pass over the
// log-posteriors: a wave per row keeps the row in registers, finds its arg-max (first index on ties) and the entry at
// the label.  partial: [waves][4] = (sum of -y[r][lab], rows whose arg-max misses the label, counted rows, bad labels).
template <int NPL>
__global__ __launch_bounds__(256) void nll_err_partial_kernel(const float* __restrict__ y, const long* __restrict__ lab,
                                                               long ignore_index, long rows, long N,
                                                               float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    float loss = 0.f, err = 0.f, cnt = 0.f, bad = 0.f;
    for (long r = wid; r < rows; r += nw) {
        const long lr = lab[r];
        const bool ignored = lr == ignore_index;
        const bool in_range = lr >= 0 && lr < N;
        float best = -INFINITY, at_lab = 0.f;
        long besti = N;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const long c = lane + 64 * i;
            const float v = c < N ? y[r * N + c] : -INFINITY;
            if (c < N && (v > best || (v == best && c < besti) || besti == N)) best = v, besti = c;  // NaN rows: index of the first column
            if (c == lr) at_lab = v;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const long oi = __shfl_xor(besti, off);
            if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
            at_lab += __shfl_xor(at_lab, off);
        }
        err += besti != lr ? 1.f : 0.f;
        if (!ignored && in_range) loss -= at_lab, cnt += 1.f;
        if (!ignored && !in_range) bad += 1.f;
    }
    if (lane == 0) {
        float* o = partial + wid * 4;
        o[0] = loss, o[1] = err, o[2] = cnt, o[3] = bad;
    }
}

// The cost of an output whose rows' arg-max positions are already known (logsoftmax_fwd_wave_kernel's amax): a lane per row,
// one gathered load (the entry at the label) and one compare - 64 000 x 1938 log-posteriors are NOT read again (0.12 ms
// of the step).  Same partial format and the same decisions as nll_err_partial_kernel.
__global__ __launch_bounds__(256) void nll_err_gather_kernel(const float* __restrict__ y, const long* __restrict__ lab,
                                                              const int* __restrict__ amax, long ignore_index, long rows,
                                                              long N, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    float loss = 0.f, err = 0.f, cnt = 0.f, bad = 0.f;
    for (long r0 = wid * 64; r0 < rows; r0 += nw * 64) {
        const long r = r0 + lane;
        if (r < rows) {
            const long lr = lab[r];
            const bool ignored = lr == ignore_index;
            const bool in_range = lr >= 0 && lr < N;
            const float at_lab = in_range ? y[r * N + lr] : 0.f;
            err += (long)amax[r] != lr ? 1.f : 0.f;
            if (!ignored && in_range) loss -= at_lab, cnt += 1.f;
            if (!ignored && !in_range) bad += 1.f;
        }
    }
    loss = pk_wave_sum(loss), err = pk_wave_sum(err), cnt = pk_wave_sum(cnt), bad = pk_wave_sum(bad);
    if (lane == 0) {
        float* o = partial + wid * 4;
        o[0] = loss, o[1] = err, o[2] = cnt, o[3] = bad;
    }
}

// out[0] = mean loss over the counted rows, out[1] = error rate over all rows, out[2] = counted rows, out[3] = bad labels
// loss_out (null or one float): a second copy of the loss (the differentiable output of functional.HeadNllFn: no device
// copy launch for it); bad_acc (null or one float): += the bad labels, in place (the chunk's persistent counter).
__global__ __launch_bounds__(256) void nll_err_final_kernel(const float* __restrict__ partial, long nw, long rows,
                                                             float* __restrict__ out, float* __restrict__ loss_out,
                                                             float* __restrict__ bad_acc) {
    __shared__ float sh[4][4];
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (long w = threadIdx.x; w < nw; w += 256) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += partial[w * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = pk_wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[threadIdx.x >> 6][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
        // 0/0 = NaN when every row is ignored, as torch.  A label outside [0, classes) trips a device-side assert in
        // torch's nll_loss; here it POISONS the loss (NaN): loud without a host sync, whoever the caller is (the count
        // in out[3] is what core.run_nn_dp turns into an exception at its next sync point)
        out[0] = t[3] > 0.f ? __builtin_nanf("") : t[0] / t[2];
        out[1] = t[1] / (float)rows;
        out[2] = t[2];
        out[3] = t[3];
        if (loss_out != nullptr) loss_out[0] = out[0];
        if (bad_acc != nullptr) bad_acc[0] += t[3];
    }
}

// ---- Block-per-row variants of the head kernels, for rows of 2049 .. 8192 columns ---------------------------------
// (every Librispeech recipe has ~3400 senones).  The wave kernels stop at 64 lanes x 32 registers; here a 256-thread
// workgroup owns a row and a thread holds up to NPT of its values: every element is still read from HBM once, all loads
// of a thread are in flight together, and the reductions are wave shuffles plus one exchange of four values through
// LDS.  Value i of thread t is column lsmb_col(i, t): with VEC (N a multiple of 4 and 16-byte aligned rows) the thread
// owns 4-column chunks, chunk j at column (j * 256 + t) * 4 - 16-byte loads, 8-byte bf16 stores, and a chunk lies
// entirely inside [0, N), [N, ldb) or beyond; without, single columns i * 256 + t.  Per-element expressions are the
// wave kernels' (the ONEHOT dz, which no cross-lane sum enters, comes out with the same bits).
template <bool VEC>
__device__ __forceinline__ long lsmb_col(int i, int t) {
    return VEC ? (long)((i >> 2) * 256 + t) * 4 + (i & 3) : (long)i * 256 + t;
}
template <int NPT, bool VEC>
__device__ __forceinline__ void lsmb_load(const float* __restrict__ row, long N, int t, float pad, float (&v)[NPT]) {
    if (VEC) {
#pragma unroll
        for (int j = 0; j < NPT / 4; ++j) {
            const long c = (long)(j * 256 + t) * 4;
            f32x4 q = {pad, pad, pad, pad};
            if (c < N) q = *(const f32x4*)(row + c);
            v[4 * j] = q[0], v[4 * j + 1] = q[1], v[4 * j + 2] = q[2], v[4 * j + 3] = q[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const long c = (long)i * 256 + t;
            v[i] = c < N ? row[c] : pad;
        }
    }
}
// sh: four floats; the caller keeps two uses of the same four apart by a barrier
__device__ __forceinline__ float lsmb_block_max(float v, float* sh) {
    v = pk_wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float lsmb_block_sum(float v, float* sh) {
    v = pk_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// contract of logsoftmax_fwd_wave_kernel (input at pitch ldx, its pad columns never read; output at pitch N; LSM_FAR;
// amax by the rule of nll_err_partial_kernel)
template <int NPT, bool VEC>
__global__ __launch_bounds__(256) void logsoftmax_fwd_block_kernel(const float* __restrict__ x, long ldx, long rows, long N,
                                                                    float* __restrict__ y, int* __restrict__ amax) {
    __shared__ float shm[4], shs[4], shb[4];
    __shared__ long shi[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        float* yr = y + r * N;
        float v[NPT];
        lsmb_load<NPT, VEC>(x + r * ldx, N, t, -INFINITY, v);
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NPT; ++i) m = fmaxf(m, v[i]);
        m = lsmb_block_max(m, shm);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) sum += expf(v[i] - m);  // exp(-inf) = 0 for the padding
        sum = lsmb_block_sum(sum, shs);  // (shm is written again behind this barrier, shs behind the next row's first)
        const float ls = logf(sum), lse = m + ls;
        const bool far = fabsf(m) > LSM_FAR;  // (see LSM_FAR)
#pragma unroll
        for (int i = 0; i < NPT; ++i) v[i] = far ? (v[i] - m) - ls : v[i] - lse;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NPT / 4; ++j) {
                const long c = (long)(j * 256 + t) * 4;
                const f32x4 q = {v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
                if (c < N) *(f32x4*)(yr + c) = q;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const long c = (long)i * 256 + t;
                if (c < N) yr[c] = v[i];
            }
        }
        if (amax != nullptr) {
            // thread 0 visits column 0 first and keeps it on a NaN row, through both merges
            float best = -INFINITY;
            long besti = N;
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const long c = lsmb_col<VEC>(i, t);
                const float u = c < N ? v[i] : -INFINITY;
                if (c < N && (u > best || (u == best && c < besti) || besti == N)) best = u, besti = c;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ob = __shfl_xor(best, off);
                const long oi = __shfl_xor(besti, off);
                if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
            }
            if (lane == 0) shb[wave] = best, shi[wave] = besti;
            __syncthreads();
            if (t == 0) {
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const float ob = shb[w];
                    const long oi = shi[w];
                    if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
                }
                amax[r] = (int)besti;
            }
            // (shb / shi are written again behind two more barriers, which thread 0 reaches after this read)
        }
    }
}

// contract of logsoftmax_bwd_bf16_kernel.  The block walks rows blockIdx.x, + gridDim.x, ...; a column has ONE owner per
// block, whose register carries its sum over those rows: the partial row needs no merge.
template <int NPT, bool VEC, bool ONEHOT>
__global__ __launch_bounds__(256) void logsoftmax_bwd_bf16_block_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                         const long* __restrict__ lab,
                                                                         const float* __restrict__ dloss,
                                                                         const float* __restrict__ count, long ignore_index,
                                                                         long rows, long N, unsigned short* __restrict__ dxb,
                                                                         long ldb, long pitch, float* __restrict__ partial) {
    __shared__ float shs[2][4];  // by row parity: one barrier per row
    const int t = threadIdx.x;
    float scale = 0.f;
    if (ONEHOT) {
        const float cnt = count[0];
        scale = cnt > 0.f ? dloss[0] / cnt : 0.f;
    }
    float acc[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) acc[i] = 0.f;
    int par = 0;
    for (long r = blockIdx.x; r < rows; r += gridDim.x, par ^= 1) {
        unsigned short* o = dxb + r * pitch;
        float g[NPT], e[NPT];
        float sum = 0.f;
        long lr = -1;
        if (ONEHOT) {
            lr = lab[r];
            if (lr == ignore_index || lr < 0 || lr >= N) lr = -1;  // (an out-of-range label is counted by the forward pass)
            sum = lr >= 0 ? -scale : 0.f;
        }
        lsmb_load<NPT, VEC>(y + r * N, N, t, -INFINITY, e);
        if (ONEHOT) {
#pragma unroll
            for (int i = 0; i < NPT; ++i) g[i] = lsmb_col<VEC>(i, t) == lr ? -scale : 0.f;
        } else {
            lsmb_load<NPT, VEC>(dy + r * N, N, t, 0.f, g);
#pragma unroll
            for (int i = 0; i < NPT; ++i) sum += g[i];
            sum = lsmb_block_sum(sum, shs[par]);
        }
        float d[NPT];
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const long c = lsmb_col<VEC>(i, t);
            d[i] = c < N ? g[i] - expf(e[i]) * sum : 0.f;
            acc[i] += d[i];
        }
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NPT / 4; ++j) {
                const long c = (long)(j * 256 + t) * 4;
                const uint2 q = {pk_pack_bf2(d[4 * j], d[4 * j + 1]), pk_pack_bf2(d[4 * j + 2], d[4 * j + 3])};
                if (c < ldb) *(uint2*)(o + c) = q;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const long c = (long)i * 256 + t;
                if (c < ldb) o[c] = pk_f2bf(d[i]);
            }
        }
    }
    // one partial row per block, in the layout col_reduce_final_kernel reads
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const long c = lsmb_col<VEC>(i, t);
        if (c < N) {
            const pk_f32x2 q = {acc[i], 0.f};
            *(pk_f32x2*)(partial + ((long)blockIdx.x * N + c) * 2) = q;
        }
    }
}

// nll_err_partial_kernel for such rows (the cost without the arg-max positions): partial [blocks][4], same decisions
template <int NPT, bool VEC>
__global__ __launch_bounds__(256) void nll_err_partial_block_kernel(const float* __restrict__ y, const long* __restrict__ lab,
                                                                     long ignore_index, long rows, long N,
                                                                     float* __restrict__ partial) {
    __shared__ float shb[2][4], sha[2][4];  // by row parity: one barrier per row
    __shared__ long shi[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float loss = 0.f, err = 0.f, cnt = 0.f, bad = 0.f;  // (thread 0's count)
    int par = 0;
    for (long r = blockIdx.x; r < rows; r += gridDim.x, par ^= 1) {
        const long lr = lab[r];
        const bool ignored = lr == ignore_index;
        const bool in_range = lr >= 0 && lr < N;
        float v[NPT];
        lsmb_load<NPT, VEC>(y + r * N, N, t, -INFINITY, v);
        float best = -INFINITY, at_lab = 0.f;
        long besti = N;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const long c = lsmb_col<VEC>(i, t);
            const float u = c < N ? v[i] : -INFINITY;
            if (c < N && (u > best || (u == best && c < besti) || besti == N)) best = u, besti = c;  // NaN rows: index of the first column
            if (c == lr) at_lab = u;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const long oi = __shfl_xor(besti, off);
            if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
            at_lab += __shfl_xor(at_lab, off);
        }
        if (lane == 0) shb[par][wave] = best, shi[par][wave] = besti, sha[par][wave] = at_lab;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float ob = shb[par][w];
                const long oi = shi[par][w];
                if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
                at_lab += sha[par][w];
            }
            err += besti != lr ? 1.f : 0.f;
            if (!ignored && in_range) loss -= at_lab, cnt += 1.f;
            if (!ignored && !in_range) bad += 1.f;
        }
    }
    if (t == 0) {
        float* o = partial + (long)blockIdx.x * 4;
        o[0] = loss, o[1] = err, o[2] = cnt, o[3] = bad;
    }
}

inline int ew_blocks(long n) {
    long b = (n + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

extern "C" int64_t pk_bn_partial_floats(int64_t M, int64_t N) { return (int64_t)row_blocks(M) * N * 3; }

extern "C" int pk_bn_stats(void* stream, const float* x, int64_t ldx, int64_t M, int64_t N, float* partial, float* mean,
                           float* var) {
    PK_REQUIRE(M > 0 && N > 0, "pk_bn_stats: empty input");
    hipStream_t st = pk_stream(stream);
    const int rb = row_blocks(M);
    if ((N & 3) == 0 && (ldx & 3) == 0 && ((uintptr_t)x & 15) == 0) {
        dim3 grid4((unsigned)((N / 4 + COLS - 1) / COLS), rb);
        hipLaunchKernelGGL(bn_stats_partial_v4_kernel, grid4, dim3(256), 0, st, x, (long)ldx, (long)M, (long)N, partial);
    } else {
        dim3 grid((unsigned)((N + COLS - 1) / COLS), rb);
        hipLaunchKernelGGL(bn_stats_partial_kernel, grid, dim3(256), 0, st, x, (long)ldx, (long)M, (long)N, partial);
    }
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)((N + FIN_COLS - 1) / FIN_COLS)), dim3(FIN_COLS * FIN_GROUPS), 0, st, partial, rb, (long)N,
                       mean, var);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_bn_finalize(void* stream, int64_t N, const float* mean, const float* var, const float* gamma,
                              const float* beta, float eps, float* scale, float* shift, float* running_mean,
                              float* running_var, float momentum, double count) {
    hipStream_t st = pk_stream(stream);
    const float unbias = count > 1.0 ? (float)(count / (count - 1.0)) : 1.0f;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (long)N, mean, var, gamma,
                       beta, eps, scale, shift, running_mean, running_var, momentum, unbias);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_bn_finalize_gates(void* stream, int G, int H, const float* mean, const float* var, const float* gamma,
                                    const float* beta, float eps, float* scale, float* shift, float* const* running_mean,
                                    float* const* running_var, int64_t* const* num_batches, float momentum, double count) {
    PK_REQUIRE(G >= 1 && G <= 4 && H >= 1, "pk_bn_finalize_gates: 1..4 gates");
    PK_REQUIRE(running_mean != nullptr && running_var != nullptr, "pk_bn_finalize_gates: null running-statistics tables");
    BnGateBufs bufs;
    for (int g = 0; g < 4; ++g) {
        bufs.rmean[g] = g < G ? running_mean[g] : nullptr;
        bufs.rvar[g] = g < G ? running_var[g] : nullptr;
        bufs.batches[g] = (g < G && num_batches != nullptr) ? (long long*)num_batches[g] : nullptr;
        PK_REQUIRE(g >= G || (bufs.rmean[g] && bufs.rvar[g]), "pk_bn_finalize_gates: null running statistics of a gate");
    }
    const float unbias = count > 1.0 ? (float)(count / (count - 1.0)) : 1.0f;
    hipLaunchKernelGGL(bn_finalize_gates_kernel, dim3((unsigned)((G * H + 255) / 256)), dim3(256), 0, pk_stream(stream), G, H,
                       mean, var, gamma, beta, eps, scale, shift, bufs, momentum, unbias);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_affine_act_fwd(void* stream, const float* x, int64_t ldx, int64_t M, int64_t N, const float* scale,
                                 const float* shift, int act, const float* mask, float* y, int64_t ldy) {
    if (M * N == 0) return 0;
    hipLaunchKernelGGL(affine_act_fwd_kernel, dim3(ew_blocks(M * N)), dim3(256), 0, pk_stream(stream), x, (long)ldx,
                       (long)M, (long)N, scale, shift, act, mask, y, (long)ldy);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_act_bwd(void* stream, const float* dy, const float* a, const float* mask, int act, int64_t n,
                          float* g) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, pk_stream(stream), dy, a, mask, act, (long)n, g);
    PK_LAUNCH_CHECK();
    return 0;
}

// the 16-byte / 8-byte forms of the exact-fp32 BatchNorm-backward passes: -> 4 / 2 when every operand is aligned to that many
// floats and N and the leading dimensions are multiples of it, else 0 (the scalar forms)
static int bn_f32_vec(int64_t N, int64_t ldg, int64_t ldx, const void* g, const void* g2, const void* x, const void* mean,
                      const void* var, const void* gamma) {
    for (int V = 4; V >= 2; V -= 2) {
        const uintptr_t m = (uintptr_t)(V * 4 - 1);
        auto al = [m](const void* p_) { return p_ == nullptr || ((uintptr_t)p_ & m) == 0; };
        if ((N % V) == 0 && (ldg % V) == 0 && (ldx % V) == 0 && al(g) && al(g2) && al(x) && al(mean) && al(var) && al(gamma)) return V;
    }
    return 0;
}

extern "C" int pk_bn_bwd_reduce(void* stream, const float* g, const float* g2, int64_t ldg, const float* x, int64_t ldx,
                                int64_t M, int64_t N, const float* mean, const float* var, float eps, float* partial,
                                float* sum_g, float* sum_gx) {
    hipStream_t st = pk_stream(stream);
    const int rb = row_blocks(M);
    const int V = bn_f32_vec(N, ldg, ldx, g, g2, x, mean, var, nullptr);
    if (V > 0) {
        dim3 vgrid((unsigned)((N + 64 * V - 1) / (64 * V)), rb);
        if (V == 4) hipLaunchKernelGGL((col_reduce_partial_vec_kernel<0, 4>), vgrid, dim3(256), 0, st, g, g2, (long)ldg, x, (long)ldx,
                                       (long)M, (long)N, mean, var, eps, partial);
        else hipLaunchKernelGGL((col_reduce_partial_vec_kernel<0, 2>), vgrid, dim3(256), 0, st, g, g2, (long)ldg, x, (long)ldx,
                                (long)M, (long)N, mean, var, eps, partial);
    } else {
        dim3 grid((unsigned)((N + COLS - 1) / COLS), rb);
        hipLaunchKernelGGL(col_reduce_partial_kernel<0>, grid, dim3(256), 0, st, g, g2, (long)ldg, x, (long)ldx, (long)M,
                           (long)N, mean, var, eps, partial);
    }
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(col_reduce_final_kernel, dim3((unsigned)((N + CF_COLS - 1) / CF_COLS)), dim3(CF_COLS * CF_GROUPS), 0, st, partial, rb, (long)N,
                       sum_g, sum_gx, (float*)nullptr, (float*)nullptr, (unsigned short*)nullptr, 0L, 0L, 0);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_bn_bwd_apply(void* stream, const float* g, const float* g2, int64_t ldg, const float* x, int64_t ldx,
                               int64_t M, int64_t N, const float* mean, const float* var, float eps, const float* gamma,
                               const float* sum_g, const float* sum_gx, double count, float* dx, int64_t lddx) {
    int V = bn_f32_vec(N, ldg, ldx, g, g2, x, mean, var, gamma);
    while (V > 0 && !((lddx % V) == 0 && ((uintptr_t)dx & (V * 4 - 1)) == 0 && ((uintptr_t)sum_g & (V * 4 - 1)) == 0 &&
                      ((uintptr_t)sum_gx & (V * 4 - 1)) == 0))
        V -= 2;
    if (V > 0) {
        dim3 vgrid((unsigned)((N + 64 * V - 1) / (64 * V)), row_blocks(M));
        if (V == 4) hipLaunchKernelGGL((bn_bwd_apply_vec_kernel<4>), vgrid, dim3(256), 0, pk_stream(stream), g, g2, (long)ldg, x,
                                       (long)ldx, (long)M, (long)N, mean, var, eps, gamma, sum_g, sum_gx, (float)(1.0 / count), dx, (long)lddx);
        else hipLaunchKernelGGL((bn_bwd_apply_vec_kernel<2>), vgrid, dim3(256), 0, pk_stream(stream), g, g2, (long)ldg, x,
                                (long)ldx, (long)M, (long)N, mean, var, eps, gamma, sum_g, sum_gx, (float)(1.0 / count), dx, (long)lddx);
    } else {
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_blocks(M * N)), dim3(256), 0, pk_stream(stream), g, g2, (long)ldg, x,
                           (long)ldx, (long)M, (long)N, mean, var, eps, gamma, sum_g, sum_gx, (float)(1.0 / count), dx,
                           (long)lddx);
    }
    PK_LAUNCH_CHECK();
    return 0;
}

// ---- backward of drop(act(bn(z))) for a SMALL batch (M <= 128 rows) in one launch: the activation / mask backward
// (pk_act_bwd), the two BatchNorm reductions (pk_bn_bwd_reduce: two launches), the BatchNorm backward itself
// (pk_bn_bwd_apply) and the bf16 conversion of its result (pk_cvt_bf16) - five launches of ~4.5 us each on a 128-frame
// MLP step whose arithmetic is 128 x 1024 elements.  A workgroup owns 32 columns and all M rows: thread (column, row
// group) keeps its g and xhat in registers between the reduction and the second pass.
//   g = dy * mask * act'(a);  sum_g = sum_rows g;  sum_gx = sum_rows g * xhat;
//   dz = gamma * invstd * (g - sum_g / M - xhat * sum_gx / M)      (neural_networks.py:139-148 backwards)
// dzb: bf16 [M][ldb] (ldb >= N; pad columns zero: the GEMM operand), dz: fp32 [M][N] or null.  sum_g / sum_gx [N] are
// written; acc_beta / acc_gamma (null or [N]): += the same sums (the parameters' .grad, accumulated in place).
// db / acc_bias (null or [N]): the column sums of dz - the gradient of the Linear bias IN FRONT of the BatchNorm, which the
// reference always creates (neural_networks.py:120) and differentiates (analytically zero; what autograd delivers is the
// rounding residue of this very sum) - written / accumulated here instead of by two more launches (pk_colsum).
// Round 4: a workgroup owns 16 columns (was 32: twice the workgroups - the launch is as long as one workgroup's footprint
// takes through its CU's memory pipe) and a thread four consecutive columns of rows rg and rg + 64 (16-byte accesses).
constexpr int SB_COLS = 16, SB_RG = 64, SB_ROWS = 2;  // 64 row groups x 2 rows = 128 rows at most
__device__ __forceinline__ f32x4 sb_rows16_sum(f32x4 v) {  // over the lanes that share (lane & 3): the 16 row groups of a wave
#pragma unroll
    for (int off = 4; off < 64; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += __shfl_xor(v[r], off, 64);
    return v;
}
__global__ __launch_bounds__(256) void bn_act_bwd_small_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                                                                const float* __restrict__ mask, int act,
                                                                const float* __restrict__ z, const float* __restrict__ mean,
                                                                const float* __restrict__ var, float eps,
                                                                const float* __restrict__ gamma, int M, int N,
                                                                unsigned short* __restrict__ dzb, long ldb,
                                                                float* __restrict__ dz, float* __restrict__ sum_g,
                                                                float* __restrict__ sum_gx, float* __restrict__ acc_beta,
                                                                float* __restrict__ acc_gamma, float* __restrict__ db,
                                                                float* __restrict__ acc_bias) {
    __shared__ float sh[3][4][SB_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c4 = (tid & 3) * 4, rg = tid >> 2;
    const int c = blockIdx.x * SB_COLS + c4;
    const bool vec = (N & 3) == 0 && (ldb & 3) == 0;  // (else: element by element)
    bool cok[4];
    float mu[4], inv[4], ga[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cok[e] = c + e < N;
        mu[e] = cok[e] ? mean[c + e] : 0.f;
        inv[e] = cok[e] ? 1.0f / sqrtf(var[c + e] + eps) : 0.f;
        ga[e] = (gamma && cok[e]) ? gamma[c + e] : 1.f;
    }
    f32x4 gv[SB_ROWS], xh[SB_ROWS];
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SB_ROWS; ++k) {
        const int r = rg + k * SB_RG;
        f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f}, x = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < M && cok[0]) {
            const long o = (long)r * N + c;
            f32x4 d, av, zv, mk = f32x4{1.f, 1.f, 1.f, 1.f};
            if (vec) {
                d = *reinterpret_cast<const f32x4*>(dy + o);
                av = *reinterpret_cast<const f32x4*>(a + o);
                zv = *reinterpret_cast<const f32x4*>(z + o);
                if (mask) mk = *reinterpret_cast<const f32x4*>(mask + o);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d[e] = cok[e] ? dy[o + e] : 0.f;
                    av[e] = cok[e] ? a[o + e] : 0.f;
                    zv[e] = cok[e] ? z[o + e] : 0.f;
                    if (mask) mk[e] = cok[e] ? mask[o + e] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                g[e] = cok[e] ? d[e] * mk[e] * pk_act_grad_from_out(act, av[e]) : 0.f;
                x[e] = cok[e] ? (zv[e] - mu[e]) * inv[e] : 0.f;
            }
        }
        gv[k] = g;
        xh[k] = x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s0[e] += g[e];
            s1[e] += g[e] * x[e];
        }
    }
    s0 = sb_rows16_sum(s0);
    s1 = sb_rows16_sum(s1);
    if (lane < 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sh[0][wave][c4 + e] = s0[e];
            sh[1][wave][c4 + e] = s1[e];
        }
    }
    __syncthreads();
    float t0[4], t1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // every thread of a column adds the four partial sums in the same order
        t0[e] = ((sh[0][0][c4 + e] + sh[0][1][c4 + e]) + sh[0][2][c4 + e]) + sh[0][3][c4 + e];
        t1[e] = ((sh[1][0][c4 + e] + sh[1][1][c4 + e]) + sh[1][2][c4 + e]) + sh[1][3][c4 + e];
    }
    if (rg == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!cok[e]) continue;
            sum_g[c + e] = t0[e];
            sum_gx[c + e] = t1[e];
            if (acc_beta) acc_beta[c + e] += t0[e];
            if (acc_gamma) acc_gamma[c + e] += t1[e];
        }
    }
    const float invM = 1.0f / (float)M;
    f32x4 s2 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SB_ROWS; ++k) {
        const int r = rg + k * SB_RG;
        if (r >= M) continue;
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d[e] = cok[e] ? ga[e] * inv[e] * (gv[k][e] - t0[e] * invM - xh[k][e] * (t1[e] * invM)) : 0.f;
            s2[e] += d[e];
        }
        if (vec && c + 3 < ldb) {
            uint2 pk;
            pk.x = pk_pack_bf2(d[0], d[1]);
            pk.y = pk_pack_bf2(d[2], d[3]);
            *reinterpret_cast<uint2*>(dzb + (long)r * ldb + c) = pk;  // (columns N .. ldb-1: zero padding)
            if (dz && cok[0]) *reinterpret_cast<f32x4*>(dz + (long)r * N + c) = d;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e < ldb) dzb[(long)r * ldb + c + e] = pk_f2bf(d[e]);
                if (dz && cok[e]) dz[(long)r * N + c + e] = d[e];
            }
        }
    }
    if (db != nullptr || acc_bias != nullptr) {  // (uniform over the grid)
        s2 = sb_rows16_sum(s2);
        if (lane < 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sh[2][wave][c4 + e] = s2[e];
        }
        __syncthreads();
        if (rg == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!cok[e]) continue;
                const float t2 = ((sh[2][0][c4 + e] + sh[2][1][c4 + e]) + sh[2][2][c4 + e]) + sh[2][3][c4 + e];
                if (db) db[c + e] = t2;
                if (acc_bias) acc_bias[c + e] += t2;
            }
        }
    }
}

extern "C" int pk_bn_act_bwd_small_covers(int64_t M, int64_t N) { return M >= 1 && M <= SB_RG * SB_ROWS && N >= 1; }
extern "C" int pk_bn_act_bwd_small(void* stream, const float* dy, const float* a, const float* mask, int act, const float* z,
                                   const float* mean, const float* var, float eps, const float* gamma, int64_t M, int64_t N,
                                   uint16_t* dzb, int64_t ldb, float* dz, float* sum_g, float* sum_gx, float* acc_beta,
                                   float* acc_gamma, float* db, float* acc_bias) {
    PK_REQUIRE(pk_bn_act_bwd_small_covers(M, N), "pk_bn_act_bwd_small: up to %d rows (got %ld x %ld)", SB_RG * SB_ROWS, (long)M, (long)N);
    PK_REQUIRE(dy && a && z && mean && var && dzb && sum_g && sum_gx && ldb >= N, "pk_bn_act_bwd_small: null argument or short pitch");
    hipLaunchKernelGGL(bn_act_bwd_small_kernel, dim3((unsigned)((ldb + SB_COLS - 1) / SB_COLS)), dim3(256), 0, pk_stream(stream), dy, a,
                       mask, act, z, mean, var, eps, gamma, (int)M, (int)N, (unsigned short*)dzb, (long)ldb, dz, sum_g, sum_gx,
                       acc_beta, acc_gamma, db, acc_bias);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_colsum(void* stream, const float* g, const float* g2, int64_t ldg, int64_t M, int64_t N,
                         float* partial, float* out) {
    hipStream_t st = pk_stream(stream);
    const int rb = row_blocks(M);
    dim3 grid((unsigned)((N + COLS - 1) / COLS), rb);
    hipLaunchKernelGGL(col_reduce_partial_kernel<1>, grid, dim3(256), 0, st, g, g2, (long)ldg, (const float*)nullptr, 0L,
                       (long)M, (long)N, (const float*)nullptr, (const float*)nullptr, 0.f, partial);
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(col_reduce_final_kernel, dim3((unsigned)((N + CF_COLS - 1) / CF_COLS)), dim3(CF_COLS * CF_GROUPS), 0, st, partial, rb, (long)N,
                       out, (float*)nullptr, (float*)nullptr, (float*)nullptr, (unsigned short*)nullptr, 0L, 0L, 0);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_add(void* stream, const float* a, const float* b, int64_t n, float* out) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(add_kernel, dim3(ew_blocks(n)), dim3(256), 0, pk_stream(stream), a, b, (long)n, out);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_layernorm_fwd(void* stream, const float* x, int64_t rows, int64_t F, const float* gamma,
                                const float* beta, float eps, float* y, float* mean, float* rinv) {
    if (rows == 0) return 0;
    PK_REQUIRE(F > 1, "pk_layernorm_fwd: needs at least 2 features (unbiased std)");
    int blocks = (int)(rows < 4096 ? rows : 4096);
    hipLaunchKernelGGL(layernorm_fwd_kernel, dim3(blocks), dim3(256), 0, pk_stream(stream), x, (long)rows, (long)F, gamma,
                       beta, eps, y, mean, rinv);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_ln_last_act_drop_fwd(void* stream, const float* z, int64_t B, int C, int L, const float* gamma,
                                       const float* beta, float eps, int act, const float* mask, float* a, float* y,
                                       float* mean, float* rinv) {
    const int64_t rows = B * C;
    if (rows == 0) return 0;
    PK_REQUIRE(L > 1, "pk_ln_last_act_drop_fwd: needs at least 2 samples per row (unbiased std)");
    PK_REQUIRE(act >= PK_ACT_LINEAR && act <= PK_ACT_ELU, "pk_ln_last_act_drop_fwd: element-wise activations only (got %d)", act);
    PK_REQUIRE((mask == nullptr) == (y == nullptr), "pk_ln_last_act_drop_fwd: y is the masked output - give both or neither");
    const int blocks = (int)((rows + 3) / 4 < 8192 ? (rows + 3) / 4 : 8192);
    hipLaunchKernelGGL(ln_last_act_drop_fwd_kernel, dim3(blocks), dim3(256), 0, pk_stream(stream), z, (long)rows, C, L, gamma,
                       beta, eps, act, mask, a, y, mean, rinv);
    PK_LAUNCH_CHECK();
    return 0;
}
extern "C" int pk_ln_last_act_drop_bwd(void* stream, const float* dy, const float* z, const float* a, const float* mask,
                                       int64_t B, int C, int L, const float* gamma, const float* mean, const float* rinv,
                                       float eps, int act, float* dz, float* pg) {
    const int64_t rows = B * C;
    if (rows == 0) return 0;
    const int blocks = (int)((rows + 3) / 4 < 8192 ? (rows + 3) / 4 : 8192);
    hipLaunchKernelGGL(ln_last_act_drop_bwd_kernel, dim3(blocks), dim3(256), 0, pk_stream(stream), dy, z, a, mask, (long)rows, C,
                       L, gamma, mean, rinv, eps, act, dz, pg);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_layernorm_bwd(void* stream, const float* dy, const float* x, int64_t rows, int64_t F,
                                const float* gamma, const float* mean, const float* rinv, float eps, float* dx,
                                float* dgx) {
    if (rows == 0) return 0;
    int blocks = (int)(rows < 4096 ? rows : 4096);
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(blocks), dim3(256), 0, pk_stream(stream), dy, x, (long)rows, (long)F,
                       gamma, mean, rinv, eps, dx, dgx);
    PK_LAUNCH_CHECK();
    return 0;
}

// fold [rb][N][3] (rows, mean, M2) partials (pk_bn_stats' own, or the ones pk_gemm_bf16_stats' epilogue wrote)
extern "C" int pk_bn_stats_merge(void* stream, const float* partial, int rb, int64_t N, float* mean, float* var) {
    PK_REQUIRE(rb > 0 && N > 0 && partial && mean && var, "pk_bn_stats_merge: bad arguments");
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)((N + FIN_COLS - 1) / FIN_COLS)), dim3(FIN_COLS * FIN_GROUPS), 0,
                       pk_stream(stream), partial, rb, (long)N, mean, var);
    PK_LAUNCH_CHECK();
    return 0;
}

// pk_bn_stats_merge + pk_bn_finalize_gates as one launch
extern "C" int pk_bn_stats_merge_finalize_gates(void* stream, const float* partial, int rb, int G, int H, float* mean, float* var,
                                                const float* gamma, const float* beta, float eps, float* scale, float* shift,
                                                float* const* running_mean, float* const* running_var,
                                                int64_t* const* num_batches, float momentum, double count) {
    PK_REQUIRE(rb > 0 && partial && mean && var && scale && shift, "pk_bn_stats_merge_finalize_gates: bad arguments");
    PK_REQUIRE(G >= 1 && G <= 4 && H >= 1, "pk_bn_stats_merge_finalize_gates: 1..4 gates");
    PK_REQUIRE(running_mean != nullptr && running_var != nullptr, "pk_bn_stats_merge_finalize_gates: null running-statistics tables");
    BnGateBufs bufs;
    for (int g = 0; g < 4; ++g) {
        bufs.rmean[g] = g < G ? running_mean[g] : nullptr;
        bufs.rvar[g] = g < G ? running_var[g] : nullptr;
        bufs.batches[g] = (g < G && num_batches != nullptr) ? (long long*)num_batches[g] : nullptr;
        PK_REQUIRE(g >= G || (bufs.rmean[g] && bufs.rvar[g]), "pk_bn_stats_merge_finalize_gates: null running statistics of a gate");
    }
    const float unbias = count > 1.0 ? (float)(count / (count - 1.0)) : 1.0f;
    const long N = (long)G * H;
    hipLaunchKernelGGL(bn_stats_final_gates_kernel, dim3((unsigned)((N + FIN_COLS - 1) / FIN_COLS)), dim3(FIN_COLS * FIN_GROUPS), 0,
                       pk_stream(stream), partial, rb, G, H, mean, var, gamma, beta, eps, scale, shift, bufs, momentum, unbias);
    PK_LAUNCH_CHECK();
    return 0;
}

#define PK_LSM_DISPATCH(KERNEL, ...)                                                                       \
    do {                                                                                                    \
        const long wblocks = (rows + 3) / 4;                                                                \
        const dim3 wgrid((unsigned)(wblocks < 16384 ? wblocks : 16384));                                    \
        if (N <= 64) hipLaunchKernelGGL((KERNEL<1>), wgrid, dim3(256), 0, st, __VA_ARGS__);                 \
        else if (N <= 256) hipLaunchKernelGGL((KERNEL<4>), wgrid, dim3(256), 0, st, __VA_ARGS__);           \
        else if (N <= 1024) hipLaunchKernelGGL((KERNEL<16>), wgrid, dim3(256), 0, st, __VA_ARGS__);         \
        else hipLaunchKernelGGL((KERNEL<32>), wgrid, dim3(256), 0, st, __VA_ARGS__);                        \
    } while (0)

// The block-per-row kernels: rows of 2049 .. 8192 columns - and, for A/B runs and the tests that compare the two families,
// every row length when PK_EXPERIMENT has head_block=1 (read per call: a test flips it inside one process).
constexpr int64_t LSM_WAVE_MAX = 2048, LSM_BLOCK_MAX = 8192;
static inline bool lsm_block_rows(int64_t N) {
    if (N > LSM_WAVE_MAX) return true;
    const char* e = pk_experiment("head_block");
    return e != nullptr && e[0] == '1';
}
static inline bool lsm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// W: the columns a block must cover (N, or the padded width a backward writes); VEC: see lsmb_col
#define PK_LSM_BLOCK_DISPATCH(W, VEC, LAUNCH)    \
    do {                                          \
        if (VEC) {                                \
            if ((W) <= 2048) LAUNCH(8, true);     \
            else if ((W) <= 4096) LAUNCH(16, true); \
            else LAUNCH(32, true);                \
        } else {                                  \
            if ((W) <= 2048) LAUNCH(8, false);    \
            else if ((W) <= 4096) LAUNCH(16, false); \
            else LAUNCH(32, false);               \
        }                                         \
    } while (0)

extern "C" int pk_logsoftmax_fwd_ld(void* stream, const float* x, int64_t ldx, int64_t rows, int64_t N, float* y) {
    if (rows == 0) return 0;
    PK_REQUIRE(ldx >= N, "pk_logsoftmax_fwd_ld: input pitch shorter than a row");
    hipStream_t st = pk_stream(stream);
    if (N <= 2048) {
        PK_LSM_DISPATCH(logsoftmax_fwd_wave_kernel, x, (long)ldx, (long)rows, (long)N, y, (int*)nullptr);
    } else {
        int blocks = (int)(rows < 8192 ? rows : 8192);
        hipLaunchKernelGGL(logsoftmax_fwd_kernel, dim3(blocks), dim3(256), 0, st, x, (long)ldx, (long)rows, (long)N, y);
    }
    PK_LAUNCH_CHECK();
    return 0;
}

// ... and the arg-max position of every output row (first index on ties), for pk_nll_err_fwd_argmax
extern "C" int pk_logsoftmax_fwd_ld_argmax(void* stream, const float* x, int64_t ldx, int64_t rows, int64_t N, float* y,
                                           int32_t* amax) {
    if (rows == 0) return 0;
    PK_REQUIRE(ldx >= N && N >= 1 && N <= LSM_BLOCK_MAX, "pk_logsoftmax_fwd_ld_argmax: rows of 1..8192 columns, pitch >= row length");
    PK_REQUIRE(x && y && amax, "pk_logsoftmax_fwd_ld_argmax: null argument");
    hipStream_t st = pk_stream(stream);
    if (lsm_block_rows(N)) {
        // a row per block and pass; ~8 resident blocks per CU, the rest of a large batch by the stride loop
        const dim3 grid((unsigned)(rows < 2048 ? rows : 2048));
        const bool vec = (N % 4) == 0 && (ldx % 4) == 0 && lsm_aligned16(x) && lsm_aligned16(y);
#define PK_LSMF(NPT, VEC) \
    hipLaunchKernelGGL((logsoftmax_fwd_block_kernel<NPT, VEC>), grid, dim3(256), 0, st, x, (long)ldx, (long)rows, (long)N, y, (int*)amax)
        PK_LSM_BLOCK_DISPATCH(N, vec, PK_LSMF);
#undef PK_LSMF
    } else {
        PK_LSM_DISPATCH(logsoftmax_fwd_wave_kernel, x, (long)ldx, (long)rows, (long)N, y, (int*)amax);
    }
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_logsoftmax_fwd(void* stream, const float* x, int64_t rows, int64_t N, float* y) {
    return pk_logsoftmax_fwd_ld(stream, x, N, rows, N, y);
}

// blocks of the fused backward: every wave keeps the column sums of its rows in registers, so the waves are long-lived -
// but a wave walks its rows one dependent HBM round trip after the other, so short rows (a 48-class head: one load per
// lane and row) need many waves to hide that: 64 000 x 48 took 284 us with 31 rows per wave, ~20 us with 4
static inline long lsm_bf16_blocks(int64_t rows, int64_t N) {
    long rows_per_wave = N <= 64 ? 4 : N <= 256 ? 8 : N <= 1024 ? 16 : 31;
    // a small batch (an MLP step of 128 frames) must not queue its rows behind one another: 128 x 1944 on 8 waves of 16
    // rows took 55 us; at least ~512 waves before a wave gets a second row
    const long spread = rows / 512 > 0 ? rows / 512 : 1;
    if (rows_per_wave > spread) rows_per_wave = spread;
    long b = (rows + 4 * rows_per_wave - 1) / (4 * rows_per_wave);
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return b;
}

// ... of the block-per-row kernel: a block is as long-lived as it can be (its threads carry the column sums), and the
// partial workspace is blocks x N x 2 floats: a row per block up to 1024 blocks (a batch of 128 frames: 128 workgroups
// on 128 CUs), beyond that the stride loop - 64 000 x 3400: 63 rows per block, 28 MB of partials next to 435 MB of dz
static inline long lsm_bf16_block_blocks(int64_t rows) { return rows < 1 ? 1 : rows < 1024 ? (long)rows : 1024; }

extern "C" int64_t pk_logsoftmax_bwd_bf16_partial_floats(int64_t rows, int64_t N) {
    return (lsm_block_rows(N) ? lsm_bf16_block_blocks(rows) : lsm_bf16_blocks(rows, N)) * N * 2;
}

static int lsm_bwd_bf16_launch(hipStream_t st, bool onehot, const float* dy, const float* y, const long* lab,
                               const float* dloss, const float* count, long ignore_index, int64_t rows, int64_t N,
                               uint16_t* dxb, int64_t ldb, float* partial, float* colsum, int64_t pitch = 0) {
    if (pitch <= 0) pitch = ldb;
    const bool block = lsm_block_rows(N);
    const long blocks = block ? lsm_bf16_block_blocks(rows) : lsm_bf16_blocks(rows, N);
    const dim3 grid((unsigned)blocks);
    unsigned short* o = (unsigned short*)dxb;
    if (block) {
        // (ldb and pitch are multiples of 8: with N a multiple of 4 every 4-column chunk of a row is 8-byte aligned in dz)
        const bool vec = (N % 4) == 0 && lsm_aligned16(y) && (onehot || lsm_aligned16(dy)) && ((uintptr_t)dxb & 7) == 0;
#define PK_LSMBB(NPT, VEC)                                                                                                     \
    do {                                                                                                                       \
        if (onehot) hipLaunchKernelGGL((logsoftmax_bwd_bf16_block_kernel<NPT, VEC, true>), grid, dim3(256), 0, st, dy, y, lab,  \
                                       dloss, count, ignore_index, (long)rows, (long)N, o, (long)ldb, (long)pitch, partial);   \
        else hipLaunchKernelGGL((logsoftmax_bwd_bf16_block_kernel<NPT, VEC, false>), grid, dim3(256), 0, st, dy, y, lab, dloss, \
                                count, ignore_index, (long)rows, (long)N, o, (long)ldb, (long)pitch, partial);                 \
    } while (0)
        PK_LSM_BLOCK_DISPATCH(ldb, vec, PK_LSMBB);
#undef PK_LSMBB
    } else {
#define PK_LSMB(NPL)                                                                                                      \
    do {                                                                                                                  \
        if (onehot) hipLaunchKernelGGL((logsoftmax_bwd_bf16_kernel<NPL, true>), grid, dim3(256), 0, st, dy, y, lab, dloss, \
                                       count, ignore_index, (long)rows, (long)N, o, (long)ldb, (long)pitch, partial);     \
        else hipLaunchKernelGGL((logsoftmax_bwd_bf16_kernel<NPL, false>), grid, dim3(256), 0, st, dy, y, lab, dloss,       \
                                count, ignore_index, (long)rows, (long)N, o, (long)ldb, (long)pitch, partial);            \
    } while (0)
    if (ldb <= 64) PK_LSMB(1);
    else if (ldb <= 256) PK_LSMB(4);
    else if (ldb <= 1024) PK_LSMB(16);
    else PK_LSMB(32);
#undef PK_LSMB
    }
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(col_reduce_final_kernel, dim3((unsigned)((N + CF_COLS - 1) / CF_COLS)), dim3(CF_COLS * CF_GROUPS), 0, st,
                       partial, (int)blocks, (long)N, colsum, (float*)nullptr, (float*)nullptr, (float*)nullptr, (unsigned short*)nullptr, 0L, 0L, 0);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_logsoftmax_bwd_bf16(void* stream, const float* dy, const float* y, int64_t rows, int64_t N, uint16_t* dxb,
                                      int64_t ldb, float* partial, float* colsum) {
    if (rows == 0) return 0;
    PK_REQUIRE(N >= 1 && N <= LSM_BLOCK_MAX, "pk_logsoftmax_bwd_bf16: rows of 1..8192 columns");
    PK_REQUIRE(ldb >= N && ldb <= LSM_BLOCK_MAX && (ldb % 8) == 0, "pk_logsoftmax_bwd_bf16: bad bf16 pitch");
    PK_REQUIRE(partial && colsum, "pk_logsoftmax_bwd_bf16: null workspace");
    return lsm_bwd_bf16_launch(pk_stream(stream), false, dy, y, nullptr, nullptr, nullptr, 0, rows, N, dxb, ldb, partial, colsum);
}

extern "C" int pk_nll_logsoftmax_bwd_bf16(void* stream, const float* y, const int64_t* lab, const float* dloss,
                                          const float* count, int64_t ignore_index, int64_t rows, int64_t N, uint16_t* dxb,
                                          int64_t ldb, float* partial, float* colsum) {
    if (rows == 0) return 0;
    PK_REQUIRE(N >= 1 && N <= LSM_BLOCK_MAX, "pk_nll_logsoftmax_bwd_bf16: rows of 1..8192 columns");
    PK_REQUIRE(ldb >= N && ldb <= LSM_BLOCK_MAX && (ldb % 8) == 0, "pk_nll_logsoftmax_bwd_bf16: bad bf16 pitch");
    PK_REQUIRE(y && lab && dloss && count && partial && colsum, "pk_nll_logsoftmax_bwd_bf16: null argument");
    return lsm_bwd_bf16_launch(pk_stream(stream), true, nullptr, y, (const long*)lab, dloss, count, (long)ignore_index, rows, N,
                               dxb, ldb, partial, colsum);
}

// ... into a column slice of a wider bf16 buffer: `ldb` columns are written per row (values + zero padding), rows are
// `pitch` elements apart
extern "C" int pk_logsoftmax_bwd_bf16_p(void* stream, const float* dy, const float* y, int64_t rows, int64_t N, uint16_t* dxb,
                                        int64_t ldb, int64_t pitch, float* partial, float* colsum) {
    if (rows == 0) return 0;
    PK_REQUIRE(N >= 1 && N <= LSM_BLOCK_MAX, "pk_logsoftmax_bwd_bf16_p: rows of 1..8192 columns");
    PK_REQUIRE(ldb >= N && ldb <= LSM_BLOCK_MAX && (ldb % 8) == 0 && pitch >= ldb && (pitch % 8) == 0, "pk_logsoftmax_bwd_bf16_p: bad bf16 pitch");
    PK_REQUIRE(partial && colsum, "pk_logsoftmax_bwd_bf16_p: null workspace");
    return lsm_bwd_bf16_launch(pk_stream(stream), false, dy, y, nullptr, nullptr, nullptr, 0, rows, N, dxb, ldb, partial, colsum, pitch);
}
extern "C" int pk_nll_logsoftmax_bwd_bf16_p(void* stream, const float* y, const int64_t* lab, const float* dloss,
                                            const float* count, int64_t ignore_index, int64_t rows, int64_t N, uint16_t* dxb,
                                            int64_t ldb, int64_t pitch, float* partial, float* colsum) {
    if (rows == 0) return 0;
    PK_REQUIRE(N >= 1 && N <= LSM_BLOCK_MAX, "pk_nll_logsoftmax_bwd_bf16_p: rows of 1..8192 columns");
    PK_REQUIRE(ldb >= N && ldb <= LSM_BLOCK_MAX && (ldb % 8) == 0 && pitch >= ldb && (pitch % 8) == 0, "pk_nll_logsoftmax_bwd_bf16_p: bad bf16 pitch");
    PK_REQUIRE(y && lab && dloss && count && partial && colsum, "pk_nll_logsoftmax_bwd_bf16_p: null argument");
    return lsm_bwd_bf16_launch(pk_stream(stream), true, nullptr, y, (const long*)lab, dloss, count, (long)ignore_index, rows, N,
                               dxb, ldb, partial, colsum, pitch);
}

static inline long nll_err_blocks(int64_t rows) {
    long b = (rows + 31) / 32;  // >= 8 rows per wave
    if (rows < 16384) b = (rows + 3) / 4;  // small batches: a row per wave (128 x 1944 on 16 waves of 8 rows took 21 us)
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return b;
}

extern "C" int64_t pk_nll_err_partial_floats(int64_t rows) { return nll_err_blocks(rows) * 4 * 4; }

extern "C" int pk_nll_err_fwd(void* stream, const float* y, const int64_t* lab, int64_t ignore_index, int64_t rows, int64_t N,
                              float* partial, float* out4, float* loss_out, float* bad_acc) {
    PK_REQUIRE(rows > 0 && N >= 1 && N <= LSM_BLOCK_MAX, "pk_nll_err_fwd: needs rows of 1..8192 columns");
    PK_REQUIRE(y && lab && partial && out4, "pk_nll_err_fwd: null argument");
    hipStream_t st = pk_stream(stream);
    const long blocks = nll_err_blocks(rows);
    const long* l = (const long*)lab;
    if (lsm_block_rows(N)) {
        // one partial entry per BLOCK: at most as many blocks as the workspace has entries for waves
        const long bb = rows < blocks * 4 ? (long)rows : blocks * 4;
        const dim3 bgrid((unsigned)bb);
        const bool vec = (N % 4) == 0 && lsm_aligned16(y);
#define PK_NLLB(NPT, VEC) \
    hipLaunchKernelGGL((nll_err_partial_block_kernel<NPT, VEC>), bgrid, dim3(256), 0, st, y, l, (long)ignore_index, (long)rows, (long)N, partial)
        PK_LSM_BLOCK_DISPATCH(N, vec, PK_NLLB);
#undef PK_NLLB
        PK_LAUNCH_CHECK();
        hipLaunchKernelGGL(nll_err_final_kernel, dim3(1), dim3(256), 0, st, partial, bb, (long)rows, out4, loss_out, bad_acc);
        PK_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid((unsigned)blocks);
    if (N <= 64) hipLaunchKernelGGL((nll_err_partial_kernel<1>), grid, dim3(256), 0, st, y, l, (long)ignore_index, (long)rows, (long)N, partial);
    else if (N <= 256) hipLaunchKernelGGL((nll_err_partial_kernel<4>), grid, dim3(256), 0, st, y, l, (long)ignore_index, (long)rows, (long)N, partial);
    else if (N <= 1024) hipLaunchKernelGGL((nll_err_partial_kernel<16>), grid, dim3(256), 0, st, y, l, (long)ignore_index, (long)rows, (long)N, partial);
    else hipLaunchKernelGGL((nll_err_partial_kernel<32>), grid, dim3(256), 0, st, y, l, (long)ignore_index, (long)rows, (long)N, partial);
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(nll_err_final_kernel, dim3(1), dim3(256), 0, st, partial, blocks * 4, (long)rows, out4, loss_out, bad_acc);
    PK_LAUNCH_CHECK();
    return 0;
}

// pk_nll_err_fwd for an output that came with its rows' arg-max positions (pk_logsoftmax_fwd_ld_argmax): same four numbers
// without reading the rows again
extern "C" int pk_nll_err_fwd_argmax(void* stream, const float* y, const int64_t* lab, const int32_t* amax, int64_t ignore_index,
                                     int64_t rows, int64_t N, float* partial, float* out4, float* loss_out, float* bad_acc) {
    PK_REQUIRE(rows > 0 && N >= 1, "pk_nll_err_fwd_argmax: empty input");
    PK_REQUIRE(y && lab && amax && partial && out4, "pk_nll_err_fwd_argmax: null argument");
    hipStream_t st = pk_stream(stream);
    long blocks = (rows + 255) / 256;  // a lane per row
    const long cap = nll_err_blocks(rows);  // (the workspace is sized by pk_nll_err_partial_floats)
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(nll_err_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, (const long*)lab, (const int*)amax,
                       (long)ignore_index, (long)rows, (long)N, partial);
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(nll_err_final_kernel, dim3(1), dim3(256), 0, st, partial, blocks * 4, (long)rows, out4, loss_out, bad_acc);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_logsoftmax_bwd_ld(void* stream, const float* dy, const float* y, int64_t rows, int64_t N, float* dx,
                                    int64_t lddx) {
    if (rows == 0) return 0;
    PK_REQUIRE(N <= 2048 && lddx >= N && lddx <= ((N + 3) & ~(int64_t)3),
               "pk_logsoftmax_bwd_ld: rows of up to 2048 classes, output pitch N rounded up to at most 4 (got N=%ld, pitch %ld)", (long)N, (long)lddx);
    hipStream_t st = pk_stream(stream);
    PK_LSM_DISPATCH(logsoftmax_bwd_wave_kernel, dy, y, (long)rows, (long)N, dx, (long)lddx);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_logsoftmax_bwd(void* stream, const float* dy, const float* y, int64_t rows, int64_t N, float* dx) {
    if (rows == 0) return 0;
    hipStream_t st = pk_stream(stream);
    if (N <= 2048) {
        PK_LSM_DISPATCH(logsoftmax_bwd_wave_kernel, dy, y, (long)rows, (long)N, dx, (long)N);
    } else {
        int blocks = (int)(rows < 8192 ? rows : 8192);
        hipLaunchKernelGGL(logsoftmax_bwd_kernel, dim3(blocks), dim3(256), 0, st, dy, y, (long)rows, (long)N, dx);
    }
    PK_LAUNCH_CHECK();
    return 0;
}
#undef PK_LSM_DISPATCH

// ---------------------------------------------------------------------------------------------
// Perf mode: BatchNorm backward straight from the bf16 gate gradients the persistent recurrence
// publishes (dGb: [ndir][M][g_pitch], gate g at column g*Hp, both directions summed here), writing
// the projection gradient as bf16 in the plain [M][G*H (+pad)] layout the dX / dW GEMMs read.
// The fp32 gate-gradient slabs are never materialised in this mode (563 MB per layer at the
// BASELINE shape).  One thread owns a 16-byte chunk (8 units of one gate) for a strip of rows.
// ---------------------------------------------------------------------------------------------
namespace {

// A block is BC_COLS chunks (of 8 columns) wide and BC_ROWL row lanes deep (BC_COLS * BC_ROWL <= 256 threads).

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // 4-byte aligned 16-byte access
__device__ __forceinline__ void ld8f(const float* p, float (&f)[8]) {
    const f32x4u a = *reinterpret_cast<const f32x4u*>(p), b = *reinterpret_cast<const f32x4u*>(p + 4);
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
    f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}
__device__ __forceinline__ void bf8_to_f32(uint4 v, float (&f)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(w[e] << 16);
        f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
    }
}

// Both passes are written so that the compiler can keep every load of an iteration in flight together: two rows per
// thread and iteration (the second one clamped to the first when the strip ends: no branch around a load), the fp32
// projection through a range-checked buffer load based at the block's first row (the 8 floats of a chunk that hangs
// over the end of a gate may run past the end of the matrix: those lanes read 0), per-column constants gathered with
// clamped indices.  The first version branched around each load (second direction? whole chunk? aligned?) and hipcc
// serialised them behind s_waitcnt vmcnt(0): three dependent HBM round trips per row and 3.3 TB/s.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bnb_rsrc(const void* p, long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0x7fffffffL ? 0x7fffffffL : bytes), 0x00020000);
}
__device__ __forceinline__ void bnb_ldx(__amdgpu_buffer_rsrc_t rs, unsigned off, float (&f)[8]) {
    const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0), b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0);
    f[0] = __uint_as_float(a[0]); f[1] = __uint_as_float(a[1]); f[2] = __uint_as_float(a[2]); f[3] = __uint_as_float(a[3]);
    f[4] = __uint_as_float(b[0]); f[5] = __uint_as_float(b[1]); f[6] = __uint_as_float(b[2]); f[7] = __uint_as_float(b[3]);
}

// MODE 0: per-column sums of g and g*xhat (BatchNorm); MODE 1: sum of g only (bias gradient, no BatchNorm)
template <int MODE, bool TWO, int BC_COLS, int BC_ROWL>
__global__ __launch_bounds__(256) void bnb_reduce_kernel(const unsigned short* __restrict__ g0,
                                                          const unsigned short* __restrict__ g1, long gpitch, int G, int H,
                                                          int Hp, const float* __restrict__ x, long ldx, long M,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          float eps, float* __restrict__ partial) {
    const int cl = threadIdx.x % BC_COLS, rl = threadIdx.x / BC_COLS;
    const int chunk = blockIdx.x * BC_COLS + cl;  // chunk index in the padded layout
    const int cpg = Hp >> 3;
    const int g = chunk / cpg, j0 = (chunk - g * cpg) * 8;
    const bool cok = g < G && rl < BC_ROWL;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    const int nvalid = cok ? ((H - j0) < 8 ? (H - j0) : 8) : 0;
    float s0[8], s1[8], mu[8], inv[8];
    {
        float vm[8], vv[8];
        const long nb = cok ? (long)g * H + j0 : 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long n = nb + (e < nvalid ? e : 0);  // clamped: every load in range, all in flight together
            vm[e] = MODE == 0 ? mean[n] : 0.f;
            vv[e] = MODE == 0 ? var[n] : 1.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s0[e] = s1[e] = 0.f;
            const bool ok = e < nvalid;
            mu[e] = (MODE == 0 && ok) ? vm[e] : 0.f;
            inv[e] = (MODE == 0 && ok) ? 1.0f / sqrtf(vv[e] + eps) : 0.f;  // inv = 0 beyond H
        }
    }
    if (cok && r0 < r1) {
        const long goff = (long)g * Hp + j0;
        const __amdgpu_buffer_rsrc_t rsx = bnb_rsrc(x + r0 * ldx, (r1 - r0) * ldx * 4);
        const unsigned xoff = (unsigned)(((long)g * H + j0) * 4), xrow = (unsigned)(ldx * 4);
        for (long r = r0 + rl; r < r1; r += 2 * BC_ROWL) {
            const bool second = r + BC_ROWL < r1;
            const long rs = second ? r + BC_ROWL : r;
            const uint4 qa0 = *reinterpret_cast<const uint4*>(g0 + r * gpitch + goff);
            const uint4 qb0 = *reinterpret_cast<const uint4*>(g0 + rs * gpitch + goff);
            uint4 qa1 = make_uint4(0, 0, 0, 0), qb1 = make_uint4(0, 0, 0, 0);
            if (TWO) {
                qa1 = *reinterpret_cast<const uint4*>(g1 + r * gpitch + goff);
                qb1 = *reinterpret_cast<const uint4*>(g1 + rs * gpitch + goff);
            }
            float xa[8], xb[8];
            if (MODE == 0) {
                bnb_ldx(rsx, (unsigned)(r - r0) * xrow + xoff, xa);
                bnb_ldx(rsx, (unsigned)(rs - r0) * xrow + xoff, xb);
            }
            __builtin_amdgcn_sched_barrier(0);  // both rows' loads are issued before anything waits for the first
            float a[8], b[8], t[8];
            bf8_to_f32(qa0, a);
            bf8_to_f32(qb0, b);
            if (TWO) {
                bf8_to_f32(qa1, t);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += t[e];
                bf8_to_f32(qb1, t);
#pragma unroll
                for (int e = 0; e < 8; ++e) b[e] += t[e];
            }
            const float w = second ? 1.f : 0.f;  // the clamped second row counts for nothing
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s0[e] += a[e];
                if (MODE == 0) s1[e] += a[e] * ((xa[e] - mu[e]) * inv[e]);
                s0[e] += w * b[e];
                if (MODE == 0) s1[e] += w * (b[e] * ((xb[e] - mu[e]) * inv[e]));
            }
        }
    }
    __shared__ float sh[BC_ROWL][BC_COLS][17];
    if (rl < BC_ROWL) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sh[rl][cl][e] = s0[e];
            sh[rl][cl][8 + e] = s1[e];
        }
    }
    __syncthreads();
    // one (chunk, element, kind) per thread and round
    for (int o = threadIdx.x; o < BC_COLS * 16; o += 256) {
        const int oc = o >> 4, oe = o & 15;
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < BC_ROWL; ++k) t += sh[k][oc][oe];
        const int ochunk = blockIdx.x * BC_COLS + oc;
        const int og = ochunk / cpg, oj = (ochunk - og * cpg) * 8 + (oe & 7);
        if (og < G && oj < H) partial[((long)blockIdx.y * ((long)G * H) + (long)og * H + oj) * 2 + (oe >> 3)] = t;
    }
}

// dx = gamma*invstd*(g - sum_g/count - xhat*sum_gx/count) as bf16 (MODE 0), or dx = g (MODE 1)
template <int MODE, bool TWO, int BC_COLS, int BC_ROWL>
__global__ __launch_bounds__(256) void bnb_apply_kernel(const unsigned short* __restrict__ g0,
                                                         const unsigned short* __restrict__ g1, long gpitch, int G, int H,
                                                         int Hp, const float* __restrict__ x, long ldx, long M,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         float eps, const float* __restrict__ gamma,
                                                         const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
                                                         float inv_count, unsigned short* __restrict__ out, long opitch) {
    const int cl = threadIdx.x % BC_COLS, rl = threadIdx.x / BC_COLS;
    const int chunk = blockIdx.x * BC_COLS + cl;
    const int cpg = Hp >> 3;
    const int g = chunk / cpg, j0 = (chunk - g * cpg) * 8;
    if (g >= G || rl >= BC_ROWL) return;
    const int rb = gridDim.y;
    const long rows_per = (M + rb - 1) / rb;
    const long r0 = (long)blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    if (r0 >= r1) return;
    const int nvalid = (H - j0) < 8 ? (H - j0) : 8;
    float mu[8], sc[8], c0[8], c1[8];
    {
        float vm[8], vv[8], vg[8], v0[8], v1[8];
        const long nb = (long)g * H + j0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long n = nb + (e < nvalid ? e : 0);
            vm[e] = MODE == 0 ? mean[n] : 0.f;
            vv[e] = MODE == 0 ? var[n] : 1.f;
            vg[e] = (MODE == 0 && gamma) ? gamma[n] : 1.f;
            v0[e] = MODE == 0 ? sum_g[n] : 0.f;
            v1[e] = MODE == 0 ? sum_gx[n] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool ok = e < nvalid;
            if (MODE == 0) {
                const float inv = 1.0f / sqrtf(vv[e] + eps);
                mu[e] = vm[e];
                sc[e] = ok ? vg[e] * inv : 0.f;
                c0[e] = v0[e] * inv_count;
                c1[e] = v1[e] * inv_count * inv;  // xhat*c1' with xhat = (x-mu)*inv folded: (x-mu)*inv*sum_gx/count
            } else {
                mu[e] = 0.f; sc[e] = ok ? 1.f : 0.f; c0[e] = 0.f; c1[e] = 0.f;
            }
        }
    }
    const long goff = (long)g * Hp + j0;
    const __amdgpu_buffer_rsrc_t rsx = bnb_rsrc(x + r0 * ldx, MODE == 0 ? (r1 - r0) * ldx * 4 : 0);
    const unsigned xoff = (unsigned)(((long)g * H + j0) * 4), xrow = (unsigned)(ldx * 4);
    const bool pairs = ((((long)g * H + j0) & 1) == 0) && ((opitch & 1) == 0);  // 4-byte aligned bf16 pairs
    for (long r = r0 + rl; r < r1; r += 2 * BC_ROWL) {
        const bool second = r + BC_ROWL < r1;
        const long rs = second ? r + BC_ROWL : r;
        const uint4 qa0 = *reinterpret_cast<const uint4*>(g0 + r * gpitch + goff);
        const uint4 qb0 = *reinterpret_cast<const uint4*>(g0 + rs * gpitch + goff);
        uint4 qa1 = make_uint4(0, 0, 0, 0), qb1 = make_uint4(0, 0, 0, 0);
        if (TWO) {
            qa1 = *reinterpret_cast<const uint4*>(g1 + r * gpitch + goff);
            qb1 = *reinterpret_cast<const uint4*>(g1 + rs * gpitch + goff);
        }
        float xa[8], xb[8];
        if (MODE == 0) {
            bnb_ldx(rsx, (unsigned)(r - r0) * xrow + xoff, xa);
            bnb_ldx(rsx, (unsigned)(rs - r0) * xrow + xoff, xb);
        }
        __builtin_amdgcn_sched_barrier(0);  // both rows' loads are issued before anything waits for the first
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half == 1 && !second) break;
            float a[8], t[8], o[8];
            bf8_to_f32(half ? qb0 : qa0, a);
            if (TWO) {
                bf8_to_f32(half ? qb1 : qa1, t);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += t[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xv = half ? xb[e] : xa[e];
                o[e] = MODE == 0 ? sc[e] * (a[e] - c0[e] - (xv - mu[e]) * c1[e]) : sc[e] * a[e];  // sc = 0 beyond H
            }
            // plain layout: column g*H + j0 (+e): 4-byte aligned pairs (H even), or single elements
            unsigned short* op = out + (half ? rs : r) * opitch + (long)g * H + j0;
            if (pairs && nvalid == 8) {
#pragma unroll
                for (int e = 0; e < 8; e += 2) *reinterpret_cast<unsigned*>(op + e) = pk_pack_bf2(o[e], o[e + 1]);
            } else {
                unsigned short hb[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) hb[e] = pk_f2bf(o[e]);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < nvalid) op[e] = hb[e];
            }
        }
    }
}

}  // namespace

extern "C" int pk_bn_bwd_bf16(void* stream, const uint16_t* g0, const uint16_t* g1, int64_t g_pitch, int G, int H,
                              const float* x, int64_t ldx, int64_t M, const float* mean, const float* var, float eps,
                              const float* gamma, double count, float* partial, float* sum_g, float* sum_gx,
                              uint16_t* out, int64_t out_pitch, float* acc_beta, float* acc_gamma) {
    PK_REQUIRE(M > 0 && G > 0 && H > 0, "pk_bn_bwd_bf16: empty input");
    PK_REQUIRE((g_pitch % 8) == 0 && ((uintptr_t)g0 & 15) == 0 && (g1 == nullptr || ((uintptr_t)g1 & 15) == 0),
               "pk_bn_bwd_bf16: gate gradients must be 16-byte aligned with a pitch that is a multiple of 8");
    PK_REQUIRE(out_pitch >= (int64_t)G * H, "pk_bn_bwd_bf16: output pitch shorter than G*H");
    hipStream_t st = pk_stream(stream);
    const int Hp = (H + 7) & ~7;
    const int chunks = G * (Hp >> 3);
    int rb = row_blocks(M);
    static int k_rbr = -1, k_rba = -1, k_cw = 0;  // development knobs (tools/bench_bnb.py): row blocks of the two passes, block width
    if (k_rbr < 0) {
        const char* e = pk_experiment("bnb_rbr"); k_rbr = e ? atoi(e) : 0;
        e = pk_experiment("bnb_rba"); k_rba = e ? atoi(e) : 0;
        e = pk_experiment("bnb_cw"); k_cw = e ? atoi(e) : 0;
    }
    if (k_rbr > 0) rb = k_rbr;
    PK_REQUIRE(((M + rb - 1) / rb) * ldx * 4 < 0x7fffffffL, "pk_bn_bwd_bf16: a row strip of the projection exceeds 2 GB");
    const int CW = k_cw == 16 ? 16 : 48;
    dim3 grid((chunks + CW - 1) / CW, rb);
    dim3 grid_a((chunks + CW - 1) / CW, k_rba > 0 ? k_rba : rb);
    const long N = (long)G * H;
    const bool use_bn = mean != nullptr;
#define PK_BNB_LAUNCH2(KERNEL, GRID, C, R, ...)                                                                           \
    do {                                                                                                                  \
        if (use_bn && g1) hipLaunchKernelGGL((KERNEL<0, true, C, R>), GRID, dim3(256), 0, st, __VA_ARGS__);               \
        else if (use_bn) hipLaunchKernelGGL((KERNEL<0, false, C, R>), GRID, dim3(256), 0, st, __VA_ARGS__);               \
        else if (g1) hipLaunchKernelGGL((KERNEL<1, true, C, R>), GRID, dim3(256), 0, st, __VA_ARGS__);                    \
        else hipLaunchKernelGGL((KERNEL<1, false, C, R>), GRID, dim3(256), 0, st, __VA_ARGS__);                           \
    } while (0)
#define PK_BNB_LAUNCH(KERNEL, GRID, ...)                                  \
    do {                                                                  \
        if (CW == 16) PK_BNB_LAUNCH2(KERNEL, GRID, 16, 16, __VA_ARGS__);  \
        else PK_BNB_LAUNCH2(KERNEL, GRID, 48, 5, __VA_ARGS__);            \
    } while (0)
    PK_BNB_LAUNCH(bnb_reduce_kernel, grid, (const unsigned short*)g0, (const unsigned short*)g1, (long)g_pitch, G, H, Hp, x,
                  (long)ldx, (long)M, mean, var, eps, partial);
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(col_reduce_final_kernel, dim3((unsigned)((N + CF_COLS - 1) / CF_COLS)), dim3(CF_COLS * CF_GROUPS), 0, st, partial, rb, N, sum_g,
                       use_bn ? sum_gx : (float*)nullptr, acc_beta, use_bn ? acc_gamma : (float*)nullptr,
                       out_pitch > N ? (unsigned short*)out : (unsigned short*)nullptr, (long)out_pitch, (long)M, (int)N);
    PK_LAUNCH_CHECK();
    PK_BNB_LAUNCH(bnb_apply_kernel, grid_a, (const unsigned short*)g0, (const unsigned short*)g1, (long)g_pitch, G, H, Hp, x,
                  (long)ldx, (long)M, mean, var, eps, gamma, sum_g, sum_gx, use_bn ? (float)(1.0 / count) : 0.f,
                  (unsigned short*)out, (long)out_pitch);
    PK_LAUNCH_CHECK();
#undef PK_BNB_LAUNCH
#undef PK_BNB_LAUNCH2
    return 0;
}
