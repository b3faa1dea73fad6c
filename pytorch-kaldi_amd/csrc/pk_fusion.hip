// pk_fusion.hip - the fusion layer of the multi-microphone Li-GRU (include/pk_amd.h: pk_fusion_fwd / pk_fusion_bwd).
//
//     pre_m[n][c] = sum_f W[c][f] x[n][m*F + f] + b[c]        P[n][c] = R_m act(pre_m[n][c])        C = 2*H0 columns
//
// A GEMM with a very short K (F = 13 in the recipe) whose epilogue is non-linear and reduces over M groups of the SAME
// rows: the [N][M][C] pre-activations live in MFMA accumulators only, P is written once, and backward recomputes them.
//
// Work split.  A workgroup is 4 waves and owns 64 rows x 64 columns; a wave owns 16 of the rows and all 64 columns (four
// 16 x 16 MFMA tiles).  The workgroup stages its 64 rows of x - all M slices, each padded with zeros to Kp = roundup(F, 16)
// - into LDS once, as bf16 in bf16 mode and as fp32 in exact mode; every microphone's operand comes from there.  The weight
// fragments of a wave's 64 columns are loaded once and stay in registers (4 tiles x Kp/16 fragments).
//
// Matrix instructions.  Both modes walk K in steps of 16 with a lane holding FOUR CONSECUTIVE k of its row / column:
// bf16 mode as one v_mfma_f32_16x16x16_bf16, exact mode as four v_mfma_f32_16x16x4_f32 (the e-th takes the lane's e-th
// value on both sides: a permutation of k that both operands share).  The 16-deep instruction, not the 32-deep one the
// recurrences use, because of what backward does with the result: a lane of the 16 x 16 accumulator holds one column and
// four consecutive rows, which is exactly an operand fragment of the 16-deep instruction with the rows as k.  So
// g_m = dP * act'(pre_m) goes from the accumulator of the first product straight into the second one (dW = g_m^T x_m over
// the wave's 16 rows; dx = g_m W with the first product taken transposed) without passing through LDS.
//
// LDS: 64 rows x (M*Kp + pad) elements <= 61 KB, i.e. M*Kp <= 480 in bf16 mode and <= 240 in exact mode; wider inputs are
// refused.  Reductions over rows (dW, db, the PReLU slopes): every wave leaves its partial in the workspace and
// fusion_reduce_kernel adds them in a fixed order - no atomics.
#include "pk_common.h"

namespace {

constexpr int FUS_THREADS = 256;  // 4 waves
constexpr int FUS_ROWS = 64;      // 16 per wave
constexpr int FUS_COLS = 64;      // 4 MFMA tiles per wave
constexpr int FUS_CT = FUS_COLS / 16;
constexpr int FUS_MAX_PARTS = 64;  // row-walking workgroups per column tile in the weight-gradient kernel

typedef short s16x4 __attribute__((ext_vector_type(4)));

// an operand fragment: four consecutive k of one row / column
template <bool BF> struct Mode;
template <> struct Mode<true> {
    typedef s16x4 Frag;
    typedef unsigned short Elem;
    static constexpr int PAD = 8;  // elements: rows stay 16-byte aligned
    static __device__ __forceinline__ short cvt(float v) { return (short)pk_f2bf(v); }
    static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float round(float v) { return pk_bf2f(pk_f2bf(v)); }
};
template <> struct Mode<false> {
    typedef f32x4 Frag;
    typedef float Elem;
    static constexpr int PAD = 4;
    static __device__ __forceinline__ float cvt(float v) { return v; }
    static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], c, 0, 0, 0);
        return c;
    }
    static __device__ __forceinline__ float round(float v) { return v; }
};

__device__ __forceinline__ float fus_act(int act, float v, float s) {
    if (act == PK_FUSION_ACT_TANH) return tanhf(v);
    if (act == PK_FUSION_ACT_RELU) return v > 0.f ? v : 0.f;
    return v > 0.f ? v : s * v;
}
__device__ __forceinline__ float fus_dact(int act, float v, float s) {
    if (act == PK_FUSION_ACT_TANH) {
        const float t = tanhf(v);
        return 1.f - t * t;
    }
    if (act == PK_FUSION_ACT_RELU) return v > 0.f ? 1.f : 0.f;
    return v > 0.f ? 1.f : s;
}
// the negative-side slope of column c: PReLU's parameter of its half, leaky_relu's 0.01
__device__ __forceinline__ float fus_slope(int act, const float* slope, int c, int H0) {
    return act == PK_FUSION_ACT_PRELU ? slope[c >= H0 ? 1 : 0] : 0.01f;
}

struct FusGeom {
    long N;
    int M, F, C, H0, act, Kp, nks, width, pitch;  // Kp = roundup(F, 16), nks = Kp / 16, width = M * Kp, pitch = width + PAD
    float rscale;                                // 1/M for the mean
};

// rows row0 .. row0+63 of x into LDS: xs[r][m*Kp + f], zeros for f >= F and rows >= N
template <bool BF>
__device__ __forceinline__ void fus_stage(const FusGeom& g, const float* __restrict__ x, long row0,
                                          typename Mode<BF>::Elem* xs) {
    const long ld = (long)g.M * g.F;
    for (int idx = threadIdx.x; idx < FUS_ROWS * g.width; idx += FUS_THREADS) {
        const int r = idx / g.width, rem = idx - r * g.width;
        const int m = rem / g.Kp, f = rem - m * g.Kp;
        const long row = row0 + r;
        const float v = (row < g.N && f < g.F) ? x[row * ld + (long)m * g.F + f] : 0.f;
        xs[r * g.pitch + rem] = (typename Mode<BF>::Elem)Mode<BF>::cvt(v);
    }
}

// the fragment of W for (row-of-W c, k-step ks): elements f = ks*16 + 4*lq + e, zeros outside [C][F]
template <bool BF>
__device__ __forceinline__ typename Mode<BF>::Frag fus_w_frag(const FusGeom& g, const float* __restrict__ W, int c, int ks, int lq) {
    typename Mode<BF>::Frag w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int f = ks * 16 + 4 * lq + e;
        w[e] = Mode<BF>::cvt((c < g.C && f < g.F) ? W[(long)c * g.F + f] : 0.f);
    }
    return w;
}

// the wave's columns: weight fragments, biases and slopes of column col0 + t*16 + (lane & 15)
template <bool BF, int NKS>
__device__ __forceinline__ void fus_load_cols(const FusGeom& g, const float* __restrict__ W, const float* __restrict__ b,
                                              const float* __restrict__ slope, int col0, int lr, int lq,
                                              typename Mode<BF>::Frag (&Wf)[FUS_CT][NKS], float (&bv)[FUS_CT], float (&sv)[FUS_CT]) {
#pragma unroll
    for (int t = 0; t < FUS_CT; ++t) {
        const int c = col0 + t * 16 + lr;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) Wf[t][ks] = fus_w_frag<BF>(g, W, c, ks, lq);
        bv[t] = c < g.C ? b[c] : 0.f;
        sv[t] = fus_slope(g.act, slope, c, g.H0);
    }
}

// pre_m - b of the wave's 16 rows x 64 columns: acc[t][r] = (row 4*lq + r, column t*16 + lr)
template <bool BF, int NKS>
__device__ __forceinline__ void fus_pre(const FusGeom& g, const typename Mode<BF>::Elem* xrow, int m,
                                        const typename Mode<BF>::Frag (&Wf)[FUS_CT][NKS], f32x4 (&acc)[FUS_CT]) {
    typedef typename Mode<BF>::Frag Frag;
#pragma unroll
    for (int t = 0; t < FUS_CT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (ks < g.nks) {
            const Frag a = *reinterpret_cast<const Frag*>(xrow + m * g.Kp + ks * 16);
#pragma unroll
            for (int t = 0; t < FUS_CT; ++t) acc[t] = Mode<BF>::mma(a, Wf[t][ks], acc[t]);
        }
    }
}

template <bool BF, int NKS>
__global__ __launch_bounds__(FUS_THREADS) void fusion_fwd_kernel(FusGeom g, const float* __restrict__ x, const float* __restrict__ W,
                                                                 const float* __restrict__ b, const float* __restrict__ slope,
                                                                 float* __restrict__ P) {
    typedef typename Mode<BF>::Frag Frag;
    typedef typename Mode<BF>::Elem Elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Elem* xs = reinterpret_cast<Elem*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    const long row0 = (long)blockIdx.x * FUS_ROWS;
    const int col0 = blockIdx.y * FUS_COLS;
    fus_stage<BF>(g, x, row0, xs);
    Frag Wf[FUS_CT][NKS];
    float bv[FUS_CT], sv[FUS_CT];
    fus_load_cols<BF, NKS>(g, W, b, slope, col0, lr, lq, Wf, bv, sv);
    __syncthreads();
    const Elem* xrow = xs + (wave * 16 + lr) * g.pitch + 4 * lq;
    f32x4 run[FUS_CT];
#pragma unroll
    for (int t = 0; t < FUS_CT; ++t) run[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < g.M; ++m) {
        f32x4 acc[FUS_CT];
        fus_pre<BF, NKS>(g, xrow, m, Wf, acc);
#pragma unroll
        for (int t = 0; t < FUS_CT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) run[t][r] += fus_act(g.act, acc[t][r] + bv[t], sv[t]);
    }
#pragma unroll
    for (int t = 0; t < FUS_CT; ++t) {
        const int c = col0 + t * 16 + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = row0 + wave * 16 + 4 * lq + r;
            if (row < g.N && c < g.C) P[row * g.C + c] = run[t][r] * g.rscale;
        }
    }
}

// Workspace of the weight-gradient kernel, in floats: parts = 4 * gridDim.x wave partials
//   dWp [parts][C][Kp] | dbp [parts][C] | dsp [parts][column tiles][2]
struct FusWs {
    long dW, db, ds, total;
    int parts, ctiles;
};
FusWs fus_ws(long N, int F, int C) {
    FusWs w;
    const long rtiles = (N + FUS_ROWS - 1) / FUS_ROWS;
    w.ctiles = (C + FUS_COLS - 1) / FUS_COLS;
    long walkers = (512 + w.ctiles - 1) / w.ctiles;  // about two workgroups per CU in all
    if (walkers > FUS_MAX_PARTS) walkers = FUS_MAX_PARTS;
    if (walkers > rtiles) walkers = rtiles;
    w.parts = (int)walkers * (FUS_THREADS / 64);
    const long Kp = (F + 15) / 16 * 16;
    w.dW = 0;
    w.db = w.dW + (long)w.parts * C * Kp;
    w.ds = w.db + (long)w.parts * C;
    w.total = w.ds + (long)w.parts * w.ctiles * 2;
    return w;
}

// dW, db and slope partials.  grid (walkers, column tiles): a workgroup keeps its columns and walks over row tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...; the sums of a wave stay in its registers until the end.
template <bool BF, int NKS>
__global__ __launch_bounds__(FUS_THREADS) void fusion_bwd_w_kernel(FusGeom g, const float* __restrict__ x, const float* __restrict__ W,
                                                                   const float* __restrict__ b, const float* __restrict__ slope,
                                                                   const float* __restrict__ dP, float* __restrict__ ws, FusWs wl,
                                                                   long rtiles) {
    typedef typename Mode<BF>::Frag Frag;
    typedef typename Mode<BF>::Elem Elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Elem* xs = reinterpret_cast<Elem*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    const int col0 = blockIdx.y * FUS_COLS;
    Frag Wf[FUS_CT][NKS];
    float bv[FUS_CT], sv[FUS_CT];
    fus_load_cols<BF, NKS>(g, W, b, slope, col0, lr, lq, Wf, bv, sv);
    f32x4 dWa[FUS_CT][NKS];  // (column t*16 + 4*lq + r, feature ks*16 + lr)
    float dbv[FUS_CT], dsv[FUS_CT];
#pragma unroll
    for (int t = 0; t < FUS_CT; ++t) {
        dbv[t] = dsv[t] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) dWa[t][ks] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const Elem* xrow = xs + (wave * 16 + lr) * g.pitch + 4 * lq;          // first product: row lr, k = 4*lq ..
    const Elem* xcol = xs + (wave * 16 + 4 * lq) * g.pitch + lr;          // second product: rows 4*lq .. as k, feature lr
    for (long rt = blockIdx.x; rt < rtiles; rt += gridDim.x) {
        const long row0 = rt * FUS_ROWS;
        __syncthreads();  // (the readers of the tile before)
        fus_stage<BF>(g, x, row0, xs);
        __syncthreads();
        f32x4 d[FUS_CT];  // dP of (row 4*lq + r, column t*16 + lr), scaled for the mean
#pragma unroll
        for (int t = 0; t < FUS_CT; ++t) {
            const int c = col0 + t * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = row0 + wave * 16 + 4 * lq + r;
                d[t][r] = (row < g.N && c < g.C) ? Mode<BF>::round(dP[row * g.C + c]) * g.rscale : 0.f;
            }
        }
        for (int m = 0; m < g.M; ++m) {
            f32x4 acc[FUS_CT];
            fus_pre<BF, NKS>(g, xrow, m, Wf, acc);
            Frag gf[FUS_CT];
#pragma unroll
            for (int t = 0; t < FUS_CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pre = acc[t][r] + bv[t];
                    const float gm = d[t][r] * fus_dact(g.act, pre, sv[t]);
                    dbv[t] += gm;
                    dsv[t] += d[t][r] * fminf(pre, 0.f);
                    gf[t][r] = Mode<BF>::cvt(gm);
                }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                if (ks < g.nks) {
                    Frag xb;
#pragma unroll
                    for (int e = 0; e < 4; ++e) xb[e] = xcol[e * g.pitch + m * g.Kp + ks * 16];
#pragma unroll
                    for (int t = 0; t < FUS_CT; ++t) dWa[t][ks] = Mode<BF>::mma(gf[t], xb, dWa[t][ks]);
                }
            }
        }
    }
    const long part = (long)blockIdx.x * (FUS_THREADS / 64) + wave;
    float* dWp = ws + wl.dW + part * g.C * g.Kp;
    float h0 = 0.f, h1 = 0.f;
#pragma unroll
    for (int t = 0; t < FUS_CT; ++t) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (ks < g.nks) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = col0 + t * 16 + 4 * lq + r;
                    if (c < g.C) dWp[(long)c * g.Kp + ks * 16 + lr] = dWa[t][ks][r];
                }
            }
        }
        const int c = col0 + t * 16 + lr;
        float v = dbv[t];  // the lane's four rows; the other twelve are in lanes lr + 16, + 32, + 48
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lq == 0 && c < g.C) ws[wl.db + part * g.C + c] = v;
        if (c < g.H0) h0 += dsv[t];
        else if (c < g.C) h1 += dsv[t];
    }
    h0 = pk_wave_sum(h0);
    h1 = pk_wave_sum(h1);
    if (lane == 0) {
        float* dsp = ws + wl.ds + (part * wl.ctiles + blockIdx.y) * 2;
        dsp[0] = h0;
        dsp[1] = h1;
    }
}

// dW [C][F], db [C] and dslope [2] from the wave partials, each sum in the order of the parts.  Blocks 0 and 1 also add up
// the slope partials of one half (thread i takes the entries i, i + 256, ..., then the wave and the four waves in order).
__global__ __launch_bounds__(256) void fusion_reduce_kernel(const float* __restrict__ ws, FusWs wl, int C, int F, int Kp, float* __restrict__ dW,
                                                            float* __restrict__ db, float* __restrict__ dslope) {
    __shared__ float wsum[4];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long nW = (long)C * F;
    if (idx < nW) {
        const long c = idx / F, f = idx - c * F;
        float s = 0.f;
        for (int p = 0; p < wl.parts; ++p) s += ws[wl.dW + ((long)p * C + c) * Kp + f];
        dW[idx] = s;
    } else if (idx < nW + C) {
        const long c = idx - nW;
        float s = 0.f;
        for (int p = 0; p < wl.parts; ++p) s += ws[wl.db + (long)p * C + c];
        db[c] = s;
    }
    if (dslope != nullptr && blockIdx.x < 2) {
        const long n = (long)wl.parts * wl.ctiles;
        float s = 0.f;
        for (long i = threadIdx.x; i < n; i += 256) s += ws[wl.ds + i * 2 + blockIdx.x];
        s = pk_wave_sum(s);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) dslope[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// dx [N][M*F] = g_m W.  One workgroup per row tile, walking over ALL columns 16 at a time, so that the sum over columns
// stays in the wave's accumulators.  The first product is taken transposed (W x_m^T: column 4*lq + r, row lr), which makes
// g_m an operand fragment of the second one with the columns as k.  W, b and dP come from L2 (W is a few KB).
template <bool BF, int NKS>
__global__ __launch_bounds__(FUS_THREADS) void fusion_bwd_x_kernel(FusGeom g, const float* __restrict__ x, const float* __restrict__ W,
                                                                   const float* __restrict__ b, const float* __restrict__ slope,
                                                                   const float* __restrict__ dP, float* __restrict__ dx) {
    typedef typename Mode<BF>::Frag Frag;
    typedef typename Mode<BF>::Elem Elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Elem* xs = reinterpret_cast<Elem*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    const long row0 = (long)blockIdx.x * FUS_ROWS;
    fus_stage<BF>(g, x, row0, xs);
    __syncthreads();
    const Elem* xrow = xs + (wave * 16 + lr) * g.pitch + 4 * lq;
    const long drow = row0 + wave * 16 + lr;  // the row whose dP this lane reads
    const long ld = (long)g.M * g.F;
    for (int m = 0; m < g.M; ++m) {
        Frag xf[NKS];
        f32x4 dxa[NKS];  // (row 4*lq + r, feature ks*16 + lr)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            dxa[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ks < g.nks) xf[ks] = *reinterpret_cast<const Frag*>(xrow + m * g.Kp + ks * 16);
        }
        for (int cc = 0; cc < g.C; cc += 16) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                if (ks < g.nks) acc = Mode<BF>::mma(fus_w_frag<BF>(g, W, cc + lr, ks, lq), xf[ks], acc);
            Frag gf;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = cc + 4 * lq + r;
                float gm = 0.f;
                if (c < g.C && drow < g.N) {
                    const float pre = acc[r] + b[c];
                    gm = Mode<BF>::round(dP[drow * g.C + c]) * g.rscale * fus_dact(g.act, pre, fus_slope(g.act, slope, c, g.H0));
                }
                gf[r] = Mode<BF>::cvt(gm);
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                if (ks < g.nks) {
                    Frag wb;  // W[column cc + 4*lq + e][feature ks*16 + lr]
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = cc + 4 * lq + e, f = ks * 16 + lr;
                        wb[e] = Mode<BF>::cvt((c < g.C && f < g.F) ? W[(long)c * g.F + f] : 0.f);
                    }
                    dxa[ks] = Mode<BF>::mma(gf, wb, dxa[ks]);
                }
            }
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int f = ks * 16 + lr;
            if (ks < g.nks && f < g.F) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = row0 + wave * 16 + 4 * lq + r;
                    if (row < g.N) dx[row * ld + (long)m * g.F + f] = dxa[ks][r];
                }
            }
        }
    }
}

int fus_geom(const char* who, int prec, int64_t N, int M, int F, int H0, int act, int mean, FusGeom* g) {
    PK_REQUIRE(prec == PK_PREC_F32 || prec == PK_PREC_BF16, "%s: precision %d (PK_PREC_F32 or PK_PREC_BF16)", who, prec);
    PK_REQUIRE(N >= 1 && M >= 1 && F >= 1 && H0 >= 1, "%s: N = %lld, M = %d, F = %d, H0 = %d must be positive", who, (long long)N,
               M, F, H0);
    PK_REQUIRE(act >= PK_FUSION_ACT_TANH && act <= PK_FUSION_ACT_PRELU, "%s: unknown activation code %d", who, act);
    PK_REQUIRE(F <= 128, "%s: F = %d features per microphone (at most 128: the weight fragments stay in registers)", who, F);
    PK_REQUIRE(H0 <= (1 << 24) && N <= (1LL << 36), "%s: N = %lld rows of 2 x %d columns are out of range", who, (long long)N, H0);
    const int Kp = (F + 15) / 16 * 16;
    const int cap = prec == PK_PREC_BF16 ? PK_FUSION_MAX_WIDTH : PK_FUSION_MAX_WIDTH / 2;
    PK_REQUIRE((long)M * Kp <= cap,
               "%s: %d microphones x %d features (padded to %d) = %ld staged values per row, above the %d a 64-row tile holds "
               "in LDS in this precision mode",
               who, M, F, Kp, (long)M * Kp, cap);
    g->N = N, g->M = M, g->F = F, g->C = 2 * H0, g->H0 = H0, g->act = act;
    g->Kp = Kp, g->nks = Kp / 16, g->width = M * Kp;
    g->pitch = g->width + (prec == PK_PREC_BF16 ? Mode<true>::PAD : Mode<false>::PAD);
    g->rscale = mean ? 1.0f / (float)M : 1.0f;
    return 0;
}

size_t fus_lds(const FusGeom& g, int prec) { return (size_t)FUS_ROWS * g.pitch * (prec == PK_PREC_BF16 ? 2 : 4); }

// the kernel template instance for (precision, k-steps): NKS is the next of 1, 2, 4, 8
#define FUS_DISPATCH(KERNEL, prec, nks, ...)                                                          \
    do {                                                                                              \
        if ((prec) == PK_PREC_BF16) {                                                                 \
            if ((nks) <= 1) FUS_LAUNCH((KERNEL<true, 1>), __VA_ARGS__);                               \
            else if ((nks) <= 2) FUS_LAUNCH((KERNEL<true, 2>), __VA_ARGS__);                          \
            else if ((nks) <= 4) FUS_LAUNCH((KERNEL<true, 4>), __VA_ARGS__);                          \
            else FUS_LAUNCH((KERNEL<true, 8>), __VA_ARGS__);                                          \
        } else {                                                                                      \
            if ((nks) <= 1) FUS_LAUNCH((KERNEL<false, 1>), __VA_ARGS__);                              \
            else if ((nks) <= 2) FUS_LAUNCH((KERNEL<false, 2>), __VA_ARGS__);                         \
            else if ((nks) <= 4) FUS_LAUNCH((KERNEL<false, 4>), __VA_ARGS__);                         \
            else FUS_LAUNCH((KERNEL<false, 8>), __VA_ARGS__);                                         \
        }                                                                                             \
    } while (0)
#define FUS_LAUNCH(K, grid, lds, st, ...) hipLaunchKernelGGL(K, grid, dim3(FUS_THREADS), lds, st, __VA_ARGS__)

}  // namespace

extern "C" int pk_fusion_fwd(void* stream, int prec, int64_t N, int M, int F, int H0, int act, int mean, const float* x,
                             const float* W, const float* b, const float* slope, float* P) {
    FusGeom g;
    if (int rc = fus_geom("pk_fusion_fwd", prec, N, M, F, H0, act, mean, &g)) return rc;
    PK_REQUIRE(x != nullptr && W != nullptr && b != nullptr && P != nullptr, "pk_fusion_fwd: x, W, b or P are NULL");
    PK_REQUIRE(act != PK_FUSION_ACT_PRELU || slope != nullptr, "pk_fusion_fwd: PReLU without its slopes");
    const dim3 grid((unsigned)((N + FUS_ROWS - 1) / FUS_ROWS), (unsigned)((g.C + FUS_COLS - 1) / FUS_COLS));
    FUS_DISPATCH(fusion_fwd_kernel, prec, g.nks, grid, fus_lds(g, prec), pk_stream(stream), g, x, W, b, slope, P);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t pk_fusion_ws_floats(int64_t N, int M, int F, int H0) {
    (void)M;
    if (N < 1 || F < 1 || H0 < 1) return 0;
    return fus_ws(N, F, 2 * H0).total;
}

extern "C" int pk_fusion_bwd(void* stream, int prec, int64_t N, int M, int F, int H0, int act, int mean, const float* x,
                             const float* W, const float* b, const float* slope, const float* dP, float* dW, float* db,
                             float* dslope, float* dx, float* ws) {
    FusGeom g;
    if (int rc = fus_geom("pk_fusion_bwd", prec, N, M, F, H0, act, mean, &g)) return rc;
    PK_REQUIRE(x != nullptr && W != nullptr && b != nullptr && dP != nullptr && dW != nullptr && db != nullptr && ws != nullptr,
               "pk_fusion_bwd: x, W, b, dP, dW, db or the workspace are NULL");
    PK_REQUIRE(act != PK_FUSION_ACT_PRELU || (slope != nullptr && dslope != nullptr), "pk_fusion_bwd: PReLU without its slopes");
    const FusWs wl = fus_ws(N, F, g.C);
    const long rtiles = (N + FUS_ROWS - 1) / FUS_ROWS;
    const dim3 wgrid((unsigned)(wl.parts / (FUS_THREADS / 64)), (unsigned)wl.ctiles);
    FUS_DISPATCH(fusion_bwd_w_kernel, prec, g.nks, wgrid, fus_lds(g, prec), pk_stream(stream), g, x, W, b, slope, dP, ws, wl, rtiles);
    PK_LAUNCH_CHECK();
    const long outs = (long)g.C * F + g.C;
    long blocks = (outs + 255) / 256;
    if (blocks < 2) blocks = 2;
    hipLaunchKernelGGL(fusion_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, pk_stream(stream), (const float*)ws, wl, g.C, F, g.Kp,
                       dW, db, act == PK_FUSION_ACT_PRELU ? dslope : nullptr);
    PK_LAUNCH_CHECK();
    if (dx != nullptr) {
        const dim3 xgrid((unsigned)rtiles);
        FUS_DISPATCH(fusion_bwd_x_kernel, prec, g.nks, xgrid, fus_lds(g, prec), pk_stream(stream), g, x, W, b, slope, dP, dx);
        PK_LAUNCH_CHECK();
    }
    return 0;
}
