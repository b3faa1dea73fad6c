// pk_sincfast.hip - SincConv_fast (neural_networks.py:1816-1959) as a fused layer: the released SincNet formula (Hz-domain
// parameters, filters normalised by 2*band, half Hamming window) with stride / padding / dilation like nn.Conv1d
// (include/pk_amd.h: pk_sincfast_bank, pk_sincfast_fwd, pk_sincfast_bwd).
//
//     y[b][c][t] = sum_k f[c][k] * x[b][t*s + k*d - p]        K odd, h = (K-1)/2, x reads as zero outside [0, n)
//     f[c][j] = f[c][K-1-j] = left[c][j] (j < h),  f[c][h] = 1
//
// Every filter is symmetric about a centre tap that is identically 1 and there is ONE input channel, so
//
//     y[b][c][t] = x[t*s + h*d - p] + sum_(j<h) left[c][j] * u[t][j],    u[t][j] = x[t*s + j*d - p] + x[t*s + (K-1-j)*d - p]
//
// and the pair sum u does not depend on the channel.  The [C][K] bank never exists on this path: only left [C][h].
//
// fp32 throughout, in every PK_PRECISION mode.  bf16 operands were decided against: fp32 direct convolution on CDNA4 is
// VALU work (the fp32 MFMA rate equals the packed-FMA rate, pk_conv.hip), and rounding raw waveforms and sinc taps to bf16
// moved a parameter gradient of the recipe-scale fixture 30 % from the reference's (the comment in
// functional.ConvPoolFn.forward).  The fold is the lever: it removes multiplies, not precision.
//
// Half-bank synthesis   sf_bank_kernel, one workgroup per filter: left [C][h], operation by operation as the reference in
//     fp32, and the [channel tile][j][CT] packed copy the convolutions read through the scalar cache (channels past C zero).
// Forward, s = d = 1    sf_fwd_fold_kernel.  grid = position tiles x batch x channel tiles.  A workgroup stages the input
//     window of its 1024 positions (+ K - 1) in LDS once, padding zeros materialised, one pad word per 64 as in pk_conv.hip
//     so that the stride-LT reads of a wave hit 64 banks.  A thread owns CT = 8 channels x LT = 4 consecutive positions.
//     The left window slides forward and the right window backward through registers: per tap pair 2 LDS words, LT adds,
//     CT scalar-cache taps and CT*LT FMAs - (1 + CT) VALU operations per position against 2*CT unfolded (9 : 16).
//     The centre tap adds x itself.  y is written once.
// Forward, other s / d  sf_fwd_plain_kernel: a wave per channel tile, a lane per position, both operands from LDS per
//     (t, j).  The position tile shrinks from 64 until (TL-1)*s + d*(K-1) + 1 words fit 64 KB.
// Filter gradient       sf_wgrad_kernel: G[c][j] = sum_(b,t) dy[b][c][t] * u[b][t][j] for j < h only - the right half is
//     the same numbers, the centre a constant.  A thread owns COT = 8 channels x JT = 4 tap pairs; a workgroup walks
//     (batch, position tile) pairs with the x window and the dy tile ([t][channel], so a thread reads its 8 channels as two
//     16-byte words) in LDS; at s = d = 1 both x windows slide forward through registers as t advances.  The reduction is
//     split over up to 256 workgroups whose partial sums sf_finish_kernel (a workgroup per filter) adds in a fixed order:
//     deterministic, no float atomics.  It then applies the analytic chain, with left_j = D_j q_j / (2 band),
//     D_j = sin(high n_j) - sin(low n_j), q_j = w_j / (n_j / 2):
//         d left_j / d high =  n_j cos(high n_j) q_j / (2 band) - left_j / band
//         d left_j / d low  = -n_j cos(low  n_j) q_j / (2 band) + left_j / band        (high held fixed)
//     high = clamp(low + min_band + |band_hz_|) passes gradient where min_low <= unclamped <= sr/2 (torch's rule, bounds
//     inclusive) and depends on low; |.| contributes sign(), 0 at 0.  These C*h terms and their sums are taken in double.
// Data gradient         only when asked for: a gather over (c, t, k) with t*s + k*d - p = i, no scatter, no atomics.
//     s = d = 1: sf_dgrad_fold_kernel, the forward loop over dy with a sum over channels (the flipped symmetric filter is
//     the filter itself); otherwise sf_dgrad_plain_kernel, folded at s = 1, with the divisibility test at s > 1.
#include <math.h>

#include <algorithm>

#include "pk_common.h"

namespace {

constexpr int SF_CT = 8, SF_LT = 4;    // forward: channels x positions of a thread
constexpr int SF_TL = 256 * SF_LT;     // positions of a workgroup of the folded kernels
constexpr int SF_COT = 8, SF_JT = 4;   // filter gradient: channels x tap pairs of a thread
constexpr int SF_WTL = 128;            // filter gradient: positions per tile (shrinks to fit the LDS)
constexpr int SF_SPLITS = 256;         // filter gradient: workgroups the reduction is split over
constexpr int SF_DCC = 8;              // data gradient: channels staged per pass (shrinks to fit the LDS)
constexpr int SF_DTI = 256;            // data gradient, plain kernel: input positions per workgroup
constexpr long SF_LDS_WORDS = 64 * 1024 / 4;

// the bank-conflict padding of pk_conv.hip: one pad word per 64
__host__ __device__ inline int sf_pad(int a) { return a + (a >> 6); }
__host__ __device__ inline long sf_padded(long words) { return (words + (words >> 6) + 4) & ~3L; }

struct SfGeom {
    long n, Lout;
    int B, C, K, h, s, p, d, ntile;
};

// neural_networks.py:1931-1947 up to the left half of band_pass / (2 * band)
__global__ __launch_bounds__(256) void sf_bank_kernel(const float* __restrict__ low_hz, const float* __restrict__ band_hz,
                                                      const float* __restrict__ n_, const float* __restrict__ window, int C, int K,
                                                      float sr, float min_low, float min_band, float* __restrict__ half,
                                                      float* __restrict__ packed) {
    const int c = blockIdx.x, h = (K - 1) / 2;
    float* pk = packed ? packed + (long)(c / SF_CT) * h * SF_CT + c % SF_CT : nullptr;
    if (c >= C) {  // the channels that fill the last tile
        for (int j = threadIdx.x; j < h; j += 256) pk[(long)j * SF_CT] = 0.f;
        return;
    }
    const float low = min_low + fabsf(low_hz[c]);
    const float high = fminf(fmaxf((low + min_band) + fabsf(band_hz[c]), min_low), sr / 2.0f);
    const float band = high - low;
    for (int j = threadIdx.x; j < h; j += 256) {
        const float nj = n_[j];
        const float v = (((sinf(high * nj) - sinf(low * nj)) / (nj / 2.0f)) * window[j]) / (2.0f * band);
        half[(long)c * h + j] = v;
        if (pk) pk[(long)j * SF_CT] = v;
    }
}

// xs[sf_pad(off + i)] = x[b][in0 + i] for i in [-off, span + off), zero outside [0, n)
__device__ __forceinline__ void sf_stage_x(const float* __restrict__ xb, long n, long in0, int span, int off, float* xs) {
    for (int i = threadIdx.x; i < span + 2 * off; i += 256) {
        const long g = in0 + i - off;
        xs[sf_pad(i)] = (g >= 0 && g < n) ? xb[g] : 0.f;
    }
}

__global__ __launch_bounds__(256) void sf_fwd_fold_kernel(SfGeom g, const float* __restrict__ x, const float* __restrict__ packed,
                                                          float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    constexpr int CT = SF_CT, LT = SF_LT;
    const int b = blockIdx.y, tile = blockIdx.z, K = g.K, h = g.h;
    const long t0 = (long)blockIdx.x * SF_TL;
    sf_stage_x(x + (long)b * g.n, g.n, t0 - g.p, SF_TL + K - 1, 0, xs);
    __syncthreads();
    const int tp = LT * threadIdx.x;
    if (t0 + tp >= g.Lout) return;
    const float* wr = packed + (long)tile * h * CT;
    float acc[CT][LT], L[LT], R[LT];  // L[i] = x[tp + i + j], R[i] = x[tp + i + K-1 - j]
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int i = 0; i < LT; ++i) acc[c][i] = 0.f;
#pragma unroll
    for (int i = 0; i < LT - 1; ++i) L[i] = xs[sf_pad(tp + i)];
#pragma unroll
    for (int i = 1; i < LT; ++i) R[i] = xs[sf_pad(tp + i + K - 1)];
#pragma unroll 4
    for (int j = 0; j < h; ++j) {
        L[LT - 1] = xs[sf_pad(tp + LT - 1 + j)];
        R[0] = xs[sf_pad(tp + K - 1 - j)];
        float u[LT];
#pragma unroll
        for (int i = 0; i < LT; ++i) u[i] = L[i] + R[i];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const float wv = wr[j * CT + c];
#pragma unroll
            for (int i = 0; i < LT; ++i) acc[c][i] = fmaf(wv, u[i], acc[c][i]);
        }
#pragma unroll
        for (int i = 0; i < LT - 1; ++i) L[i] = L[i + 1];
#pragma unroll
        for (int i = LT - 1; i > 0; --i) R[i] = R[i - 1];
    }
    float xc[LT];
#pragma unroll
    for (int i = 0; i < LT; ++i) xc[i] = xs[sf_pad(tp + i + h)];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int ch = tile * CT + c;
        if (ch >= g.C) break;
        float* yr = y + ((long)b * g.C + ch) * g.Lout + t0 + tp;
#pragma unroll
        for (int i = 0; i < LT; ++i)
            if (t0 + tp + i < g.Lout) yr[i] = acc[c][i] + xc[i];
    }
}

// any stride / dilation: a wave per channel tile, a lane per position (TL <= 64 positions per workgroup)
__global__ __launch_bounds__(256) void sf_fwd_plain_kernel(SfGeom g, int TL, const float* __restrict__ x,
                                                           const float* __restrict__ packed, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    constexpr int CT = SF_CT;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, K = g.K, h = g.h, s = g.s, d = g.d;
    const long t0 = (long)blockIdx.x * TL;
    sf_stage_x(x + (long)b * g.n, g.n, t0 * s - g.p, (TL - 1) * s + (K - 1) * d + 1, 0, xs);
    __syncthreads();
    const int tile = blockIdx.z * 4 + wave;
    if (tile >= g.ntile || lane >= TL || t0 + lane >= g.Lout) return;
    const float* wr = packed + (long)tile * h * CT;
    const int base = lane * s;
    float acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.f;
    for (int j = 0; j < h; ++j) {
        const float u = xs[sf_pad(base + j * d)] + xs[sf_pad(base + (K - 1 - j) * d)];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = fmaf(wr[j * CT + c], u, acc[c]);
    }
    const float xc = xs[sf_pad(base + h * d)];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int ch = tile * CT + c;
        if (ch < g.C) y[((long)b * g.C + ch) * g.Lout + t0 + lane] = acc[c] + xc;
    }
}

// ---- filter gradient ------------------------------------------------------------------------------------------------
// A unit is (channel group cg of COT, tap-pair group jg of JT), unit = cg * njg + jg; workgroup blockIdx.y owns the units
// [blockIdx.y * upb, + upb), one per thread, and stages the dy rows of the channel groups they touch.
struct SfWgrad {
    int TL, ntl, njg, nunits, upb, ny, nch, splits;
    long lds_words;
};

template <bool SLIDE>
__global__ __launch_bounds__(256) void sf_wgrad_kernel(SfGeom g, SfWgrad w, const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int COT = SF_COT, JT = SF_JT;
    const int tid = threadIdx.x, K = g.K, h = g.h, s = g.s, d = g.d, TL = w.TL;
    const int u0 = blockIdx.y * w.upb, unit = u0 + tid;
    const bool active = tid < w.upb && unit < w.nunits;
    const int cg = unit / w.njg, j0 = (unit - cg * w.njg) * JT;
    const int cg_lo = u0 / w.njg, cg_hi = (min(u0 + w.upb, w.nunits) - 1) / w.njg;
    const int ch_lo = cg_lo * COT, nch = (cg_hi - cg_lo + 1) * COT, pitch = nch + 4;
    const int span = (TL - 1) * s + (K - 1) * d + 1;
    const int XO = SLIDE ? JT : 0;  // slack on both sides: the tap pairs past h of the last group (computed, dropped) stay inside the allocation
    float* xs = smem;
    float* dys = smem + sf_padded(span + 2 * XO);
    const int cl0 = (cg - cg_lo) * COT;
    float acc[COT][JT];
#pragma unroll
    for (int c = 0; c < COT; ++c)
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) acc[c][jj] = 0.f;
    const long npairs = (long)g.B * w.ntl;
    for (long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
        const int b = (int)(pair / w.ntl);
        const long t0 = (pair - (long)b * w.ntl) * TL;
        __syncthreads();
        sf_stage_x(x + (long)b * g.n, g.n, t0 * s - g.p, span, XO, xs);
        for (int idx = tid; idx < nch * TL; idx += 256) {
            const int cl = idx / TL, t = idx - cl * TL, ch = ch_lo + cl;
            dys[t * pitch + cl] = (ch < g.C && t0 + t < g.Lout) ? dy[((long)b * g.C + ch) * g.Lout + t0 + t] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        float L[JT], R[JT];  // SLIDE: L[jj] = x[t + j0 + jj], R[jj] = x[t + K-1 - j0 - jj]: both move forward with t
        if (SLIDE) {
#pragma unroll
            for (int jj = 0; jj < JT - 1; ++jj) L[jj] = xs[sf_pad(XO + j0 + jj)];
#pragma unroll
            for (int jj = 1; jj < JT; ++jj) R[jj] = xs[sf_pad(XO + K - 1 - j0 - jj)];
        }
#pragma unroll 2
        for (int t = 0; t < TL; ++t) {
            float u[JT];
            if (SLIDE) {
                L[JT - 1] = xs[sf_pad(XO + t + j0 + JT - 1)];
                R[0] = xs[sf_pad(XO + t + K - 1 - j0)];
#pragma unroll
                for (int jj = 0; jj < JT; ++jj) u[jj] = L[jj] + R[jj];
#pragma unroll
                for (int jj = 0; jj < JT - 1; ++jj) L[jj] = L[jj + 1];
#pragma unroll
                for (int jj = JT - 1; jj > 0; --jj) R[jj] = R[jj - 1];
            } else {
#pragma unroll
                for (int jj = 0; jj < JT; ++jj) {
                    const int j = min(j0 + jj, h - 1);  // (the pairs past h are computed and dropped)
                    u[jj] = xs[sf_pad(t * s + j * d)] + xs[sf_pad(t * s + (K - 1 - j) * d)];
                }
            }
            const f32x4 da = *reinterpret_cast<const f32x4*>(dys + t * pitch + cl0);
            const f32x4 db = *reinterpret_cast<const f32x4*>(dys + t * pitch + cl0 + 4);
#pragma unroll
            for (int c = 0; c < COT; ++c) {
                const float dv = c < 4 ? da[c] : db[c - 4];
#pragma unroll
                for (int jj = 0; jj < JT; ++jj) acc[c][jj] = fmaf(dv, u[jj], acc[c][jj]);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int c = 0; c < COT; ++c) {
        const int ch = cg * COT + c;
#pragma unroll
        for (int jj = 0; jj < JT; ++jj)
            if (ch < g.C && j0 + jj < h) partial[((long)blockIdx.x * g.C + ch) * h + j0 + jj] = acc[c][jj];
    }
}

// partial [splits][C][h] -> dlow [C], dband [C]
__global__ __launch_bounds__(256) void sf_finish_kernel(const float* __restrict__ partial, int splits, const float* __restrict__ low_hz,
                                                        const float* __restrict__ band_hz, const float* __restrict__ n_,
                                                        const float* __restrict__ window, const float* __restrict__ half, int C,
                                                        int K, float sr, float min_low, float min_band, float* __restrict__ dlow,
                                                        float* __restrict__ dband) {
    __shared__ double sh[2][256];
    const int c = blockIdx.x, tid = threadIdx.x, h = (K - 1) / 2;
    const float lz = low_hz[c], bz = band_hz[c];
    const float low = min_low + fabsf(lz);
    const float unclamped = (low + min_band) + fabsf(bz);
    const float high = fminf(fmaxf(unclamped, min_low), sr / 2.0f);
    const double band = (double)high - (double)low;
    double ghi = 0.0, glo = 0.0;
    for (int j = tid; j < h; j += 256) {
        double G = 0.0;
        for (int sp = 0; sp < splits; ++sp) G += (double)partial[((long)sp * C + c) * h + j];
        const double nj = n_[j], q = (double)window[j] / (nj / 2.0), lf = half[(long)c * h + j];
        ghi += G * (nj * cos((double)high * nj) * q / (2.0 * band) - lf / band);
        glo += G * (-nj * cos((double)low * nj) * q / (2.0 * band) + lf / band);
    }
    sh[0][tid] = ghi;
    sh[1][tid] = glo;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            sh[0][tid] += sh[0][tid + off];
            sh[1][tid] += sh[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double pass = (unclamped >= min_low && unclamped <= sr / 2.0f) ? 1.0 : 0.0;  // torch.clamp backward
        const double gh = sh[0][0] * pass;
        dlow[c] = (float)((lz > 0.f ? 1.0 : (lz < 0.f ? -1.0 : 0.0)) * (sh[1][0] + gh));  // torch.abs backward: sign, 0 at 0
        dband[c] = (float)((bz > 0.f ? 1.0 : (bz < 0.f ? -1.0 : 0.0)) * gh);
    }
}

// ---- data gradient ----------------------------------------------------------------------------------------------------
// s = d = 1: dx[i] = sum_c ( dy[c][i+p-h] + sum_(j<h) left[c][j] (dy[c][i+p-j] + dy[c][i+p-(K-1)+j]) ).  With the window
// starting at t = i0 + p - (K-1), a thread at ip reads dys[ip + ii + K-1 - j] and dys[ip + ii + j]: the forward loop.
__global__ __launch_bounds__(256) void sf_dgrad_fold_kernel(SfGeom g, int CC, const float* __restrict__ dy, const float* __restrict__ half,
                                                            float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LT = SF_LT;
    const int tid = threadIdx.x, b = blockIdx.y, K = g.K, h = g.h;
    const long i0 = (long)blockIdx.x * SF_TL, tlo = i0 + g.p - (K - 1);
    const int span = SF_TL + K - 1, spanp = (int)sf_padded(span), ip = LT * tid;
    float acc[LT] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < g.C; c0 += CC) {
        const int ncc = min(CC, g.C - c0);
        __syncthreads();
        for (int cl = 0; cl < ncc; ++cl) sf_stage_x(dy + ((long)b * g.C + c0 + cl) * g.Lout, g.Lout, tlo, span, 0, smem + cl * spanp);
        __syncthreads();
        if (i0 + ip >= g.n) continue;
        for (int cl = 0; cl < ncc; ++cl) {
            const float* dr = smem + cl * spanp;
            const float* wr = half + (long)(c0 + cl) * h;
            float L[LT], R[LT];
#pragma unroll
            for (int i = 0; i < LT - 1; ++i) L[i] = dr[sf_pad(ip + i)];
#pragma unroll
            for (int i = 1; i < LT; ++i) R[i] = dr[sf_pad(ip + i + K - 1)];
#pragma unroll 4
            for (int j = 0; j < h; ++j) {
                L[LT - 1] = dr[sf_pad(ip + LT - 1 + j)];
                R[0] = dr[sf_pad(ip + K - 1 - j)];
                const float wv = wr[j];
#pragma unroll
                for (int i = 0; i < LT; ++i) acc[i] = fmaf(wv, L[i] + R[i], acc[i]);
#pragma unroll
                for (int i = 0; i < LT - 1; ++i) L[i] = L[i + 1];
#pragma unroll
                for (int i = LT - 1; i > 0; --i) R[i] = R[i - 1];
            }
#pragma unroll
            for (int i = 0; i < LT; ++i) acc[i] += dr[sf_pad(ip + i + h)];
        }
    }
#pragma unroll
    for (int i = 0; i < LT; ++i)
        if (i0 + ip + i < g.n) dx[(long)b * g.n + i0 + ip + i] = acc[i];
}

// any stride / dilation: a thread per input position; the dy window [tlo, tlo + tspan) of CC channels in LDS
__global__ __launch_bounds__(256) void sf_dgrad_plain_kernel(SfGeom g, int CC, int tspan, const float* __restrict__ dy,
                                                             const float* __restrict__ half, float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, b = blockIdx.y, K = g.K, h = g.h, s = g.s, d = g.d;
    const long i0 = (long)blockIdx.x * SF_DTI, lo = i0 + g.p - (long)(K - 1) * d;
    const long tlo = lo >= 0 ? lo / s : -((-lo + s - 1) / s);  // floor(lo / s)
    const int spanp = (int)sf_padded(tspan);
    const long i = i0 + tid;
    float acc = 0.f;
    for (int c0 = 0; c0 < g.C; c0 += CC) {
        const int ncc = min(CC, g.C - c0);
        __syncthreads();
        for (int cl = 0; cl < ncc; ++cl) sf_stage_x(dy + ((long)b * g.C + c0 + cl) * g.Lout, g.Lout, tlo, tspan, 0, smem + cl * spanp);
        __syncthreads();
        for (int cl = 0; cl < ncc; ++cl) {
            const float* dr = smem + cl * spanp;
            const float* wr = half + (long)(c0 + cl) * h;
            if (s == 1) {  // folded: t = i + p - k*d for k = j and k = K-1-j
                const int q = (int)(i + g.p - tlo);
                for (int j = 0; j < h; ++j) acc = fmaf(wr[j], dr[sf_pad(q - j * d)] + dr[sf_pad(q - (K - 1 - j) * d)], acc);
                acc += dr[sf_pad(q - h * d)];
            } else {
                for (int k = 0; k < K; ++k) {
                    const long num = i + g.p - (long)k * d;
                    if (num < 0 || num % s != 0) continue;
                    const float f = k == h ? 1.f : wr[k < h ? k : K - 1 - k];
                    acc = fmaf(f, dr[sf_pad((int)(num / s - tlo))], acc);
                }
            }
        }
    }
    if (i < g.n) dx[(long)b * g.n + i] = acc;
}

int sf_geom(const char* who, int B, int64_t n, int C, int K, int s, int p, int d, SfGeom& g) {
    PK_REQUIRE(C >= 1 && C <= (1 << 16), "%s: C = %d filters (1 .. 65536)", who, C);
    PK_REQUIRE(K >= 3 && (K & 1) == 1 && K <= (1 << 16), "%s: K = %d taps (odd - SincConv_fast makes it so -, 3 .. 65535)", who, K);
    PK_REQUIRE(s >= 1 && s <= (1 << 16) && d >= 1 && d <= (1 << 16), "%s: stride %d, dilation %d (1 .. 65536 each)", who, s, d);
    PK_REQUIRE(p >= 0 && p <= (1 << 24), "%s: padding %d (0 .. 2^24)", who, p);
    PK_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d sentences (1 .. 65535)", who, B);
    PK_REQUIRE(n >= 1 && n <= (1LL << 30), "%s: n = %lld samples (1 .. 2^30)", who, (long long)n);
    const long num = (long)n + 2L * p - (long)d * (K - 1) - 1;
    PK_REQUIRE(num >= 0, "%s: no output position: n + 2p - d(K-1) - 1 = %lld + 2*%d - %d*%d - 1 < 0", who, (long long)n, p, d, K - 1);
    g.n = n, g.Lout = num / s + 1;
    g.B = B, g.C = C, g.K = K, g.h = (K - 1) / 2, g.s = s, g.p = p, g.d = d, g.ntile = (C + SF_CT - 1) / SF_CT;
    return 0;
}

bool sf_fold_fits(const SfGeom& g) { return g.s == 1 && g.d == 1 && sf_padded(SF_TL + g.K - 1) <= SF_LDS_WORDS; }

int sf_wgrad_geom(const char* who, const SfGeom& g, SfWgrad& w) {
    w.njg = (g.h + SF_JT - 1) / SF_JT;
    w.nunits = (g.C + SF_COT - 1) / SF_COT * w.njg;
    w.ny = (w.nunits + 255) / 256;
    w.upb = (w.nunits + w.ny - 1) / w.ny;
    const int ncg = (g.C + SF_COT - 1) / SF_COT;
    w.nch = std::min((w.upb + w.njg - 2) / w.njg + 1, ncg) * SF_COT;  // channel rows a workgroup's units can touch
    const int xo = (g.s == 1 && g.d == 1) ? SF_JT : 0;
    for (w.TL = SF_WTL;; w.TL /= 2) {
        w.lds_words = sf_padded((long)(w.TL - 1) * g.s + (long)(g.K - 1) * g.d + 1 + 2 * xo) + (long)w.TL * (w.nch + 4);
        if (w.lds_words <= SF_LDS_WORDS || w.TL == 1) break;
    }
    PK_REQUIRE(w.lds_words <= SF_LDS_WORDS,
               "%s: the filter gradient needs %ld bytes of LDS for one position (d*(K-1) = %d*%d input words and %d channel "
               "rows; 65536 bytes at most)", who, w.lds_words * 4, g.d, g.K - 1, w.nch);
    w.ntl = (int)((g.Lout + w.TL - 1) / w.TL);
    w.splits = (int)std::min((long)SF_SPLITS, (long)g.B * w.ntl);
    return 0;
}

}  // namespace

extern "C" int64_t pk_sincfast_work_floats(int C, int K) {
    if (C < 1 || K < 3) return 0;
    return (int64_t)((C + SF_CT - 1) / SF_CT) * ((K - 1) / 2) * SF_CT;
}

extern "C" int pk_sincfast_bank(void* stream, const float* low_hz, const float* band_hz, const float* n_, const float* window, int C,
                                int K, float sample_rate, float min_low_hz, float min_band_hz, float* half, float* packed) {
    PK_REQUIRE(C >= 1 && C <= (1 << 16), "pk_sincfast_bank: C = %d filters (1 .. 65536)", C);
    PK_REQUIRE(K >= 3 && (K & 1) == 1 && K <= (1 << 16), "pk_sincfast_bank: K = %d taps (odd, 3 .. 65535)", K);
    PK_REQUIRE(low_hz && band_hz && n_ && window && half, "pk_sincfast_bank: low_hz, band_hz, n_, window or half are NULL");
    const int blocks = packed ? (C + SF_CT - 1) / SF_CT * SF_CT : C;
    hipLaunchKernelGGL(sf_bank_kernel, dim3(blocks), dim3(256), 0, pk_stream(stream), low_hz, band_hz, n_, window, C, K, sample_rate,
                       min_low_hz, min_band_hz, half, packed);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_sincfast_fwd(void* stream, const float* x, const float* packed, int B, int64_t n, int C, int K, int s, int p, int d,
                               float* y) {
    SfGeom g;
    if (int rc = sf_geom("pk_sincfast_fwd", B, n, C, K, s, p, d, g)) return rc;
    const bool fold = sf_fold_fits(g);
    int TL = fold ? SF_TL : 64;  // the plain kernel's position tile shrinks until its window fits
    long words = sf_padded(SF_TL + K - 1);
    while (!fold && (words = sf_padded((long)(TL - 1) * s + (long)(K - 1) * d + 1)) > SF_LDS_WORDS && TL > 1) TL /= 2;
    PK_REQUIRE(words <= SF_LDS_WORDS, "pk_sincfast_fwd: the input window of ONE output position, d*(K-1) + 1 = %d*%d + 1 words "
               "(%ld bytes), does not fit 65536 bytes of LDS", d, K - 1, words * 4);
    PK_REQUIRE(x && packed && y, "pk_sincfast_fwd: x, packed or y are NULL");
    const long tiles = (g.Lout + TL - 1) / TL;
    if (fold) {
        hipLaunchKernelGGL(sf_fwd_fold_kernel, dim3((unsigned)tiles, B, g.ntile), dim3(256), words * 4, pk_stream(stream), g, x, packed, y);
    } else {
        hipLaunchKernelGGL(sf_fwd_plain_kernel, dim3((unsigned)tiles, B, (g.ntile + 3) / 4), dim3(256), words * 4, pk_stream(stream), g,
                           TL, x, packed, y);
    }
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t pk_sincfast_partial_floats(int B, int64_t n, int C, int K, int s, int p, int d) {
    SfGeom g;
    SfWgrad w;
    if (sf_geom("pk_sincfast_partial_floats", B, n, C, K, s, p, d, g) || sf_wgrad_geom("pk_sincfast_partial_floats", g, w)) return 0;
    return (int64_t)w.splits * C * g.h;
}

extern "C" int pk_sincfast_bwd(void* stream, const float* x, const float* dy, const float* low_hz, const float* band_hz,
                               const float* n_, const float* window, const float* half, int B, int64_t n, int C, int K, int s, int p,
                               int d, float sample_rate, float min_low_hz, float min_band_hz, float* dlow, float* dband, float* dx,
                               float* partial) {
    SfGeom g;
    SfWgrad w;
    if (int rc = sf_geom("pk_sincfast_bwd", B, n, C, K, s, p, d, g)) return rc;
    if (int rc = sf_wgrad_geom("pk_sincfast_bwd", g, w)) return rc;
    PK_REQUIRE(x && dy && low_hz && band_hz && n_ && window && half && dlow && dband && partial,
               "pk_sincfast_bwd: an argument other than dx is NULL");
    const bool slide = s == 1 && d == 1;
    hipLaunchKernelGGL(slide ? sf_wgrad_kernel<true> : sf_wgrad_kernel<false>, dim3(w.splits, w.ny), dim3(256), w.lds_words * 4,
                       pk_stream(stream), g, w, x, dy, partial);
    PK_LAUNCH_CHECK();
    hipLaunchKernelGGL(sf_finish_kernel, dim3(C), dim3(256), 0, pk_stream(stream), (const float*)partial, w.splits, low_hz, band_hz, n_,
                       window, half, C, K, sample_rate, min_low_hz, min_band_hz, dlow, dband);
    PK_LAUNCH_CHECK();
    if (!dx) return 0;
    int CC = std::min(SF_DCC, C);
    if (sf_fold_fits(g)) {
        const long row = sf_padded(SF_TL + K - 1);
        while (CC > 1 && CC * row > SF_LDS_WORDS) CC /= 2;
        hipLaunchKernelGGL(sf_dgrad_fold_kernel, dim3((unsigned)((n + SF_TL - 1) / SF_TL), B), dim3(256), CC * row * 4, pk_stream(stream),
                           g, CC, dy, half, dx);
    } else {
        const long tspan = ((long)SF_DTI - 1 + (long)(K - 1) * d) / s + 2, row = sf_padded(tspan);
        while (CC > 1 && CC * row > SF_LDS_WORDS) CC /= 2;
        PK_REQUIRE(row <= SF_LDS_WORDS, "pk_sincfast_bwd: the data gradient's window of one channel, (255 + d*(K-1))/s + 2 = (255 + "
                   "%d*%d)/%d + 2 words (%ld bytes), does not fit 65536 bytes of LDS", d, K - 1, s, row * 4);
        hipLaunchKernelGGL(sf_dgrad_plain_kernel, dim3((unsigned)((n + SF_DTI - 1) / SF_DTI), B), dim3(256), CC * row * 4,
                           pk_stream(stream), g, CC, (int)tspan, dy, half, dx);
    }
    PK_LAUNCH_CHECK();
    return 0;
}
