// pk_logmel.hip - the raw-audio front-end (include/pk_amd.h: pk_logmel_fwd, pk_chavg_fwd / pk_chavg_bwd).
//
//     re, im [row][k] = sum_n x[frame*hop + n][b] * basis[n][k]          row = (frame, sentence b), k < n_freq = ws/2 + 1
//     y[frame][b][m]  = log10(max(sum_k fb[k][m] * (re^2 + im^2), 1e-20))
//
// Two chained products with a non-linear step between them; re, im and the power never leave registers, x is read once
// and y is written once.
//
// Work split.  x[t][b] lies at t*B + b, so the 16 rows of an MFMA tile are SB = min(16, roundup_pow2(B)) SENTENCES at
// FT = 16 / SB consecutive frame indices: row r is sentence b0 + r % SB at frame (tile's first) + r / SB.  A workgroup
// owns one group of SB sentences and NW * R row tiles (NW waves of R tiles each: NW * R * FT frames).  It stages the time
// slab those frames span, [span][SB] floats, from HBM into LDS as it lies in memory - 64-byte pieces at SB = 16, no
// transposition - and every wave walks over ALL frequency tiles for its own R row tiles, so that the sum over
// frequencies of the second product stays in the wave's accumulators.  The operand fragment of a row tile is then
// xs[(frame offset * hop + n) * SB + sentence]: at SB = 16 the 64 lanes of a K step read 64 consecutive LDS words.
//
// Matrix instruction: v_mfma_f32_16x16x4_f32 for both products, in every precision mode (bf16 operands would put a noise
// floor 54 dB under each frame's peak).  The first product is taken transposed - basis^T (16 frequencies x 4 samples)
// times x^T (4 samples x 16 rows) - which leaves frequency 4*lq + r of row lr in element r of lane (lr, lq) of the re and
// the im accumulator alike.  power[r] = re[r]^2 + im[r]^2 is therefore, for e = 0..3, an A fragment (row lr, k = lq) of
// the second product if its e-th K = 4 instruction takes frequency 4*lq + e on both sides: a permutation of k that the
// fb fragment shares (the trick of pk_fusion.hip).  The result is (row 4*lq + r, mel lr): 16 lanes store 64 contiguous
// bytes of y.
//
// basis comes in the layout this kernel streams (functional.logmel_basis builds it): [Kp][NFT * 32] fp32, Kp = roundup(ws,
// 16), NFT = ceil(n_freq / 16), column ft*32 + 2*j + c = component c (0: w cos, 1: -w sin) of frequency ft*16 + j; rows
// n >= ws and frequencies >= n_freq are zero.  A lane loads re and im of its frequency as one 8-byte word, a K step of a
// wave is four full 128-byte lines, and the loads of the next 16 samples are in flight while the current 16 multiply.
// basis (665 KB at ws = 400) and fb live in L2 / L1; the fb fragments of a frequency tile are loaded once per tile, in
// front of its K loop, and serve the wave's R row tiles.
//
// LDS: span * SB * 4 bytes, span = (NW*R*FT - 1) * hop + Kp.  The host takes the largest of (NW, R) = (4, 2), (4, 1),
// (2, 1), (1, 1) that fits 64 KB and still gives a workgroup to every CU, else the smallest; (1, 1) never needs more than
// 64 KB inside the covered range, so there is no opt-in to more.  (A 97 KB slab - (4, 2) at ws = 400, hop = 160 - was
// measured: one workgroup per CU, a wave per SIMD, 0.34 ms against the 0.28 ms of (4, 1) with its two workgroups per CU.)
#include "pk_common.h"

namespace {

constexpr int LM_MAX_WS = 1024, LM_MAX_MELS = 128, LM_MT = LM_MAX_MELS / 16, LM_KB = 16;  // LM_KB: samples per basis block
constexpr size_t LM_LDS_MAX = 64 * 1024;  // two workgroups per CU measured faster than one with a larger slab
constexpr long LM_FILL = 256;  // workgroups below which a smaller split is taken (one per CU of an MI355X)

struct LmGeom {
    long T, frames;
    int B, ws, hop, nfreq, nmels, Kp, nft, nmt, SB, sbshift, FT, span;
};

__device__ __forceinline__ f32x4 lm_mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the basis block (frequency tile ft, samples kb*16 ..): w[s] = (re, im) of sample kb*16 + 4*s + lq, frequency ft*16 + lr
__device__ __forceinline__ void lm_load_basis(const LmGeom& g, const float2* __restrict__ basis2, int ft, int kb, int lr, int lq,
                                              float2 (&w)[LM_KB / 4]) {
    const long pitch = (long)g.nft * 16;  // float2 per row
    const float2* p = basis2 + ((long)kb * LM_KB + lq) * pitch + ft * 16 + lr;
#pragma unroll
    for (int s = 0; s < LM_KB / 4; ++s) w[s] = p[(long)s * 4 * pitch];
}

// the x operands of block kb: v[s][j] = sample kb*16 + 4*s + lq of row lr of row tile j (xoff carries lq, lr and j); the
// samples past the window inside the last block read as zero whatever lies there (their basis rows are zero as well)
template <int R>
__device__ __forceinline__ void lm_load_x(const LmGeom& g, const float* xs, const int (&xoff)[R], int kb, int lq, float (&v)[LM_KB / 4][R]) {
#pragma unroll
    for (int s = 0; s < LM_KB / 4; ++s) {
        const int n = kb * LM_KB + 4 * s;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const float t = xs[xoff[j] + n * g.SB];
            v[s][j] = n + lq < g.ws ? t : 0.f;
        }
    }
}

template <int R>
__global__ __launch_bounds__(256) void logmel_kernel(LmGeom g, const float* __restrict__ x, const float* __restrict__ basis,
                                                     const float* __restrict__ fb, float* __restrict__ y, int vec) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, lr = lane & 15, lq = lane >> 4;
    const int fpw = nw * R * g.FT;  // frames of this workgroup
    const long f0 = (long)blockIdx.x * fpw;
    const int b0 = blockIdx.y * g.SB;
    const long t0 = f0 * g.hop;
    // the slab xs[tt][bb] = x[t0 + tt][b0 + bb], zero beyond T and B
    if (vec) {  // B % 4 == 0, SB >= 4, x 16-byte aligned: four sentences per load
        const int q = g.SB >> 2;
        for (int idx = threadIdx.x; idx < g.span * q; idx += blockDim.x) {
            const int tt = idx / q, b4 = (idx - tt * q) * 4;
            const long t = t0 + tt;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < g.T && b0 + b4 < g.B) v = *reinterpret_cast<const f32x4*>(x + t * g.B + b0 + b4);
            *reinterpret_cast<f32x4*>(xs + tt * g.SB + b4) = v;
        }
    } else {
        for (int idx = threadIdx.x; idx < g.span * g.SB; idx += blockDim.x) {
            const int tt = idx >> g.sbshift, bb = idx & (g.SB - 1);
            const long t = t0 + tt;
            xs[idx] = (t < g.T && b0 + bb < g.B) ? x[t * g.B + b0 + bb] : 0.f;
        }
    }
    __syncthreads();
    // first product, B operand: row lr of row tile j = sentence lr % SB at frame offset (wave*R + j)*FT + lr / SB
    int xoff[R];
#pragma unroll
    for (int j = 0; j < R; ++j) xoff[j] = (((wave * R + j) * g.FT + (lr >> g.sbshift)) * g.hop + lq) * g.SB + (lr & (g.SB - 1));
    const float2* basis2 = reinterpret_cast<const float2*>(basis);
    const int nkb = g.Kp / LM_KB;
    f32x4 yacc[R][LM_MT];  // (row 4*lq + r, mel mt*16 + lr)
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int mt = 0; mt < LM_MT; ++mt) yacc[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the operands of the next block of 16 samples - basis from L2, x from LDS - are loaded while the current block multiplies
    float2 wn[LM_KB / 4];
    float xn[LM_KB / 4][R];
    lm_load_basis(g, basis2, 0, 0, lr, lq, wn);
    lm_load_x<R>(g, xs, xoff, 0, lq, xn);
    for (int ft = 0; ft < g.nft; ++ft) {
        // fb fragments of this frequency tile: element e = fb[ft*16 + 4*lq + e][mt*16 + lr], zero outside
        f32x4 fbf[LM_MT];
#pragma unroll
        for (int mt = 0; mt < LM_MT; ++mt) {
            if (mt < g.nmt) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = ft * 16 + 4 * lq + e, m = mt * 16 + lr;
                    const bool in = k < g.nfreq && m < g.nmels;
                    const float t = fb[in ? k * g.nmels + m : 0];
                    fbf[mt][e] = in ? t : 0.f;
                }
            }
        }
        f32x4 re[R], im[R];  // (frequency ft*16 + 4*lq + r, row lr)
#pragma unroll
        for (int j = 0; j < R; ++j) re[j] = im[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nkb; ++kb) {
            float2 w[LM_KB / 4];
            float xv[LM_KB / 4][R];
#pragma unroll
            for (int s = 0; s < LM_KB / 4; ++s) {
                w[s] = wn[s];
#pragma unroll
                for (int j = 0; j < R; ++j) xv[s][j] = xn[s][j];
            }
            // (after the very last block: that block once more, which keeps the loop free of branches)
            const bool wrap = kb + 1 == nkb;
            const int kbn = wrap ? (ft + 1 < g.nft ? 0 : kb) : kb + 1, ftn = wrap && ft + 1 < g.nft ? ft + 1 : ft;
            lm_load_basis(g, basis2, ftn, kbn, lr, lq, wn);
            lm_load_x<R>(g, xs, xoff, kbn, lq, xn);
#pragma unroll
            for (int s = 0; s < LM_KB / 4; ++s) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    re[j] = lm_mma(w[s].x, xv[s][j], re[j]);
                    im[j] = lm_mma(w[s].y, xv[s][j], im[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            f32x4 pw;
#pragma unroll
            for (int e = 0; e < 4; ++e) pw[e] = re[j][e] * re[j][e] + im[j][e] * im[j][e];
#pragma unroll
            for (int mt = 0; mt < LM_MT; ++mt) {
                if (mt < g.nmt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) yacc[j][mt] = lm_mma(pw[e], fbf[mt][e], yacc[j][mt]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * lq + r;
            const long frame = f0 + (wave * R + j) * g.FT + (row >> g.sbshift);
            const int b = b0 + (row & (g.SB - 1));
            if (frame < g.frames && b < g.B) {
                float* yr = y + (frame * g.B + b) * g.nmels;
#pragma unroll
                for (int mt = 0; mt < LM_MT; ++mt) {
                    const int m = mt * 16 + lr;
                    if (mt < g.nmt && m < g.nmels) yr[m] = log10f(fmaxf(yacc[j][mt][r], 1e-20f));
                }
            }
        }
    }
}

// ---- channel averaging: y[n] = sum_c x[n][c] w[c].  A workgroup copies 256 rows - one contiguous piece of x - into LDS
// with 16-byte loads where x is aligned (rows padded to an odd pitch), then a thread adds up one row.
constexpr int CH_ROWS = 256;

__global__ __launch_bounds__(CH_ROWS) void chavg_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, long N, int C,
                                                            int vec, float* __restrict__ y) {
    __shared__ float tile[CH_ROWS * (PK_CHAVG_MAX_C + 1)];
    const long row0 = (long)blockIdx.x * CH_ROWS;
    const int rows = N - row0 < CH_ROWS ? (int)(N - row0) : CH_ROWS;
    const int n = rows * C, pitch = C | 1;
    const float* src = x + row0 * C;  // (a multiple of 256 floats from x)
    if (vec) {
        for (int i = threadIdx.x * 4; i < n; i += CH_ROWS * 4) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (i + 3 < n) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(src + i);
                v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
            } else {
                for (int e = 0; i + e < n; ++e) v[e] = src[i + e];
            }
            for (int e = 0; e < 4 && i + e < n; ++e) {
                const int r = (i + e) / C;
                tile[r * pitch + (i + e - r * C)] = v[e];
            }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += CH_ROWS) {
            const int r = i / C;
            tile[r * pitch + (i - r * C)] = src[i];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += tile[threadIdx.x * pitch + c] * w[c];
        y[row0 + threadIdx.x] = s;
    }
}

// dx[n][c] = dy[n] w[c], four consecutive elements of the flat [N*C] array per thread
__global__ __launch_bounds__(256) void chavg_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ w, long total, int C, int vec,
                                                        float* __restrict__ dx) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    const long r = i / C;
    int c = (int)(i - r * C);
    long row = r;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = i + e < total ? dy[row] * w[c] : 0.f;
        if (++c == C) c = 0, ++row;
    }
    if (vec && i + 3 < total) {
        *reinterpret_cast<f32x4*>(dx + i) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (int e = 0; e < 4 && i + e < total; ++e) dx[i + e] = v[e];
    }
}

int chavg_geom(const char* who, int64_t N, int C) {
    PK_REQUIRE(C >= 1 && C <= PK_CHAVG_MAX_C, "%s: C = %d channels (1 .. %d: a 256-row tile is staged in LDS)", who, C, PK_CHAVG_MAX_C);
    PK_REQUIRE(N >= 1 && N <= (1LL << 40) / C, "%s: N = %lld rows of %d channels (N * C in 1 .. 2^40)", who, (long long)N, C);
    return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int pk_logmel_fwd(void* stream, const float* x, const float* basis, const float* fb, int64_t T, int B, int ws, int hop,
                             int n_mels, float* y) {
    PK_REQUIRE(ws >= 4 && ws <= LM_MAX_WS, "pk_logmel_fwd: window size %d (4 .. %d)", ws, LM_MAX_WS);
    PK_REQUIRE(hop >= 1 && hop <= ws, "pk_logmel_fwd: shift %d for a window of %d (1 .. the window size)", hop, ws);
    PK_REQUIRE(n_mels >= 1 && n_mels <= LM_MAX_MELS, "pk_logmel_fwd: %d mel filters (1 .. %d)", n_mels, LM_MAX_MELS);
    PK_REQUIRE(T >= ws, "pk_logmel_fwd: T = %lld samples are shorter than one window of %d", (long long)T, ws);
    PK_REQUIRE(B >= 1 && B <= (1 << 19), "pk_logmel_fwd: B = %d sentences (1 .. 2^19)", B);
    PK_REQUIRE(T <= (1LL << 40) / B, "pk_logmel_fwd: T * B = %lld * %d samples are out of range (2^40)", (long long)T, B);
    PK_REQUIRE(x != nullptr && basis != nullptr && fb != nullptr && y != nullptr, "pk_logmel_fwd: x, basis, fb or y are NULL");
    LmGeom g;
    g.T = T, g.B = B, g.ws = ws, g.hop = hop, g.nmels = n_mels;
    g.frames = 1 + (T - ws) / hop;
    g.nfreq = ws / 2 + 1;
    g.Kp = (ws + LM_KB - 1) / LM_KB * LM_KB;
    g.nft = (g.nfreq + 15) / 16;
    g.nmt = (n_mels + 15) / 16;
    g.SB = 1, g.sbshift = 0;
    while (g.SB < 16 && g.SB < B) g.SB *= 2, ++g.sbshift;
    g.FT = 16 / g.SB;
    const long stiles = (B + g.SB - 1) / g.SB;
    static const int splits[4][2] = {{4, 2}, {4, 1}, {2, 1}, {1, 1}};  // (waves, row tiles per wave)
    int nw = 1, R = 1;
    for (int i = 0; i < 4; ++i) {
        nw = splits[i][0], R = splits[i][1];
        const long fpw = (long)nw * R * g.FT;
        const size_t lds = (size_t)((fpw - 1) * hop + g.Kp) * g.SB * sizeof(float);
        if (lds <= LM_LDS_MAX && (g.frames + fpw - 1) / fpw * stiles >= LM_FILL) break;
    }
    const long fpw = (long)nw * R * g.FT;
    g.span = (int)((fpw - 1) * hop + g.Kp);
    const size_t lds = (size_t)g.span * g.SB * sizeof(float);
    const long ftiles = (g.frames + fpw - 1) / fpw;
    PK_REQUIRE(lds <= LM_LDS_MAX, "pk_logmel_fwd: a slab of %zu bytes does not fit the LDS", lds);  // (cannot happen in range)
    PK_REQUIRE(ftiles < (1LL << 31), "pk_logmel_fwd: %lld frame tiles are more than a grid holds", (long long)ftiles);
    const void* k = R == 2 ? (const void*)logmel_kernel<2> : (const void*)logmel_kernel<1>;
    int vec = g.SB >= 4 && B % 4 == 0 && aligned16(x);
    void* args[] = {&g, &x, &basis, &fb, &y, &vec};
    PK_CHECK_HIP(hipLaunchKernel(k, dim3((unsigned)ftiles, (unsigned)stiles), dim3(64 * nw), args, lds, pk_stream(stream)));
    return 0;
}

extern "C" int pk_chavg_fwd(void* stream, const float* x, const float* w, int64_t N, int C, float* y) {
    if (int rc = chavg_geom("pk_chavg_fwd", N, C)) return rc;
    PK_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "pk_chavg_fwd: x, w or y are NULL");
    const long blocks = (N + CH_ROWS - 1) / CH_ROWS;
    hipLaunchKernelGGL(chavg_fwd_kernel, dim3((unsigned)blocks), dim3(CH_ROWS), 0, pk_stream(stream), x, w, (long)N, C, (int)aligned16(x), y);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_chavg_bwd(void* stream, const float* dy, const float* w, int64_t N, int C, float* dx) {
    if (int rc = chavg_geom("pk_chavg_bwd", N, C)) return rc;
    PK_REQUIRE(dy != nullptr && w != nullptr && dx != nullptr, "pk_chavg_bwd: dy, w or dx are NULL");
    const long total = (long)N * C, blocks = (total + 1023) / 1024;
    hipLaunchKernelGGL(chavg_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, pk_stream(stream), dy, w, total, C, (int)aligned16(dx), dx);
    PK_LAUNCH_CHECK();
    return 0;
}
