// pk_sru.hip - the time scan of a Simple Recurrent Unit layer (Lei et al., 2018; the v2 cell of the `sru` package that the
// reference's SRU class wraps, neural_networks.py:1973-2020), forward and backward, both directions in one launch each.
//
// All matrix work of an SRU layer is one time-parallel GEMM (U = x~ . W, functional.linear).  What is left is, for every
// (sentence b, direction d, unit j) column, a strictly sequential chain over T steps that touches no other column:
//
//     f   = sigmoid(u1 + v_f * c_prev + b_f)            u_g = U[t][b][(d*H + j)*k + g]   (k = 3 or 4, innermost)
//     r   = sigmoid(u2 + v_r * c_prev + b_r)
//     c   = u0 + (c_prev - u0) * f                      c_{-1} = 0;  direction 1 walks t = T-1 .. 0
//     h   = x' + (act(c) * m_h - x') * r                x' = u3 (k = 4) | scale_x * x[t][b][col] (k = 3, skip) | 0
//
// Work split: ONE THREAD PER COLUMN b*out + d*H + j (out = ndir*H), 64-thread workgroups (one wave each, so that the
// 2200 waves of the 128 x 1100 shape spread evenly over the 1024 SIMDs).  c, v_f, v_r, b_f, b_r, the masks (and, backward,
// dc and the four running parameter sums) stay in registers for all T steps.  No LDS, no MFMA, nothing is exchanged.
// H = 550 is no multiple of 64: a wave may straddle the direction and the sentence boundary, so direction, sentence
// length and therefore the time index are per thread.
//
// Loads.  A step of a thread is one 16-byte load of U for k = 4, one 12-byte load at a 12-byte pitch for k = 3 (declared
// 4-byte aligned: right for every H and out), plus 4 bytes each of x / C / dY where they are read.  Neighbouring lanes read
// neighbouring addresses.
//
// Latency.  At the recipe's shape (B = 8: 8800 columns, 138 waves on 1024 SIMDs) occupancy hides nothing: the only thing
// that overlaps a load with arithmetic is the thread's own run-ahead.  Every thread therefore keeps a REGISTER RING of
// SRU_P steps: the loads of step s + SRU_P are issued before the arithmetic of step s, the ring slot index is a
// compile-time constant after unrolling, and the wait in front of step s is for the oldest outstanding load only (vmcnt
// counts in order).  Blocks of SRU_P steps whose steps, and the next block's, all exist run without a guard or branch;
// the rest of the walk (and all of it for T < 2 * SRU_P) runs a guarded copy of the block.  SRU_P = 8: the backward ring
// is 8 x 7 VGPRs, the compiler's allocation 125 .. 168, so the kernels are bounded to 3 waves per SIMD - the 128 x 1100
// shape then has its 2200 waves resident on the 1024 SIMDs in a single pass, with 140800 x 8 x 28 B = 31 MB in flight,
// above the bandwidth x latency product of HBM.  At B = 8 a step costs latency / 8 (measured: 256 ns).  Twice the depth
// would halve that and cost a second pass at the large shape (2 waves per SIMD).
//
// Backward reads U, C (the saved c_t), x, dY and recomputes f, r, act(c).  Direction 0 walks T-1 .. 0, direction 1 walks
// 0 .. T-1.  dU is written OVER U: element (t, col, g) of dU depends on U only through elements of the same thread that it
// has already loaded.  dv_f, dv_r, db_f, db_r leave as per-sentence partial sums [B][4*out] (pk_colsum reduces them over b:
// deterministic, no atomics).  All element offsets are 64-bit (T*B*out*k*4 bytes passes 4 GB at T = 1000, B = 128).
//
// lens (forward only): sentence b has L_b steps (clamped into 0 .. T); direction 0 runs t < L_b, direction 1 starts at
// L_b - 1, rows t >= L_b of Y (and Ym) are written as zeros.
#include "pk_common.h"

namespace {

constexpr int SRU_P = 8;         // steps of run-ahead per thread (register ring)
constexpr int SRU_THREADS = 64;  // one wave per workgroup

struct SruU3 {  // 12 bytes, 4-byte aligned
    float a, b, c;
};

template <int K> __device__ __forceinline__ void sru_load_u(const float* p, float (&u)[4]) {
    if (K == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        u[0] = v[0], u[1] = v[1], u[2] = v[2], u[3] = v[3];
    } else {
        const SruU3 v = *reinterpret_cast<const SruU3*>(p);
        u[0] = v.a, u[1] = v.b, u[2] = v.c, u[3] = 0.0f;
    }
}
template <int K> __device__ __forceinline__ void sru_store_u(float* p, float d0, float d1, float d2, float d3) {
    if (K == 4) {
        *reinterpret_cast<f32x4*>(p) = f32x4{d0, d1, d2, d3};
    } else {
        *reinterpret_cast<SruU3*>(p) = SruU3{d0, d1, d2};
    }
}

constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f;
constexpr float SELU_SCALE = 1.0507009873554804934193349852946f;

__device__ __forceinline__ float sru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float sru_act(int act, float c) {
    switch (act) {
        case PK_SRU_ACT_TANH: return tanhf(c);
        case PK_SRU_ACT_RELU: return c > 0.0f ? c : 0.0f;
        case PK_SRU_ACT_SELU: return SELU_SCALE * (c > 0.0f ? c : SELU_ALPHA * (expf(c) - 1.0f));
        default: return c;
    }
}
// act(c) and its derivative, both from c
__device__ __forceinline__ float sru_act_grad(int act, float c, float& g) {
    switch (act) {
        case PK_SRU_ACT_TANH: g = tanhf(c); return 1.0f - g * g;
        case PK_SRU_ACT_RELU: g = c > 0.0f ? c : 0.0f; return c > 0.0f ? 1.0f : 0.0f;
        case PK_SRU_ACT_SELU: {
            const float e = SELU_ALPHA * expf(c);
            g = SELU_SCALE * (c > 0.0f ? c : e - SELU_ALPHA);
            return SELU_SCALE * (c > 0.0f ? 1.0f : e);
        }
        default: g = c; return 1.0f;
    }
}

// Column geometry of a thread: sentence b, column col of [out], direction, walk length n.
struct SruCol {
    long gid;   // b*out + col: the offset of the column in a [B][out] row block
    long step;  // B*out: elements between consecutive t of a [T*B][out] tensor
    int col, dir, n;
};
__device__ __forceinline__ bool sru_col(int T, int B, int H, int out, const int32_t* __restrict__ lens, SruCol& q) {
    q.step = (long)B * out;
    q.gid = (long)blockIdx.x * SRU_THREADS + threadIdx.x;
    if (q.gid >= q.step) return false;
    const int b = (int)(q.gid / out);
    q.col = (int)(q.gid - (long)b * out);
    q.dir = q.col >= H ? 1 : 0;
    q.n = T;
    if (lens != nullptr) {
        const int L = lens[b];
        q.n = L < 0 ? 0 : (L > T ? T : L);
    }
    return true;
}

// What a thread keeps for all T steps next to its state.
struct SruPar {
    float vf, vr, bf, br, m, mn, scale_x;
    int act;
};

// SRU_P steps of the forward scan, s0 .. s0 + SRU_P - 1, of one thread; e is the element offset of step s0 in a
// [T*B][out] tensor and moves along.  FULL: all of these steps and all of the next block's exist - no guard, no branch
// between the loads, so that the only waits are the counted ones in front of each step's arithmetic.
template <int K, bool HASX, bool FULL>
__device__ __forceinline__ void sru_fwd_block(const float* __restrict__ U, const float* __restrict__ x, float* __restrict__ Y,
                                              float* __restrict__ C, float* __restrict__ Ym, const SruPar& p, long& e, long de,
                                              int s0, int n, float (&ru)[SRU_P][4], float (&rx)[SRU_P], float& c) {
#pragma unroll
    for (int i = 0; i < SRU_P; ++i) {
        const int s = s0 + i;
        if (FULL || s < n) {
            const float u0 = ru[i][0], u1 = ru[i][1], u2 = ru[i][2], u3 = ru[i][3], xv = rx[i];
            if (FULL || s + SRU_P < n) {  // the ring slot is free: step s + SRU_P goes in flight before this step's arithmetic
                const long ea = e + SRU_P * de;
                sru_load_u<K>(U + ea * K, ru[i]);
                if (HASX) rx[i] = x[ea];
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the scheduler from gathering the block's loads at its top (a second ring)
            const float f = sru_sigmoid(u1 + p.vf * c + p.bf);
            const float r = sru_sigmoid(u2 + p.vr * c + p.br);
            c = u0 + (c - u0) * f;
            const float xp = K == 4 ? u3 : (HASX ? p.scale_x * xv : 0.0f);
            const float h = xp + (sru_act(p.act, c) * p.m - xp) * r;
            Y[e] = h;
            if (C != nullptr) C[e] = c;
            if (Ym != nullptr) Ym[e] = h * p.mn;
            e += de;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int K, bool HASX>
__global__ void __launch_bounds__(SRU_THREADS, 3) pk_sru_fwd_kernel(const float* __restrict__ U, const float* __restrict__ x,
                                                                    float scale_x, const float* __restrict__ wc,
                                                                    const float* __restrict__ bias, const float* __restrict__ mh,
                                                                    const int32_t* __restrict__ lens,
                                                                    const float* __restrict__ mnext, int T, int B, int H,
                                                                    int out, int act, float* __restrict__ Y,
                                                                    float* __restrict__ C, float* __restrict__ Ym) {
    SruCol q;
    if (!sru_col(T, B, H, out, lens, q)) return;
    const SruPar p = {wc[q.col], wc[out + q.col], bias[q.col], bias[out + q.col], mh != nullptr ? mh[q.gid] : 1.0f,
                      mnext != nullptr ? mnext[q.gid] : 1.0f, scale_x, act};
    const int n = q.n;
    // element offset of walk index s in a [T*B][out] tensor: direction 0 walks up, direction 1 down from n - 1
    long e = q.dir ? (long)(n - 1) * q.step + q.gid : q.gid;
    const long de = q.dir ? -q.step : q.step;

    float ru[SRU_P][4], rx[SRU_P];
    if (n > 0) {
#pragma unroll
        for (int i = 0; i < SRU_P; ++i) {  // branch-free: a slot behind the last step re-reads the last step and is never used
            const long ea = e + (i < n ? i : n - 1) * de;
            sru_load_u<K>(U + ea * K, ru[i]);
            rx[i] = HASX ? x[ea] : 0.0f;
        }
    }
    float c = 0.0f;
    int s0 = 0;
    for (; s0 + 2 * SRU_P < n; s0 += SRU_P) sru_fwd_block<K, HASX, true>(U, x, Y, C, Ym, p, e, de, s0, n, ru, rx, c);
    for (; s0 < n; s0 += SRU_P) sru_fwd_block<K, HASX, false>(U, x, Y, C, Ym, p, e, de, s0, n, ru, rx, c);
    for (int t = n; t < T; ++t) {  // padding rows of a shorter sentence
        const long ez = (long)t * q.step + q.gid;
        Y[ez] = 0.0f;
        if (C != nullptr) C[ez] = 0.0f;
        if (Ym != nullptr) Ym[ez] = 0.0f;
    }
}

// The same for the backward scan.  DYS: bit 0 = dY is there, bit 1 = dYm is there (dy = dY + dYm * mask_next).  A ring
// slot of step s holds U, x and the output gradients of its row, and c_prev = C of the row of step s + 1 (0 behind the
// last step).  FULL: additionally step s + SRU_P + 1 exists for every s of the block.
template <int K, bool HASX, int DYS, bool FULL>
__device__ __forceinline__ void sru_bwd_block(float* U, const float* __restrict__ C, const float* __restrict__ x,
                                              const float* __restrict__ dY, const float* __restrict__ dYm,
                                              float* __restrict__ dxs, const SruPar& p, long& e, long de, int s0, int T,
                                              float (&ru)[SRU_P][4], float (&rx)[SRU_P], float (&rc)[SRU_P],
                                              float (&rdy)[SRU_P], float (&rdm)[SRU_P], float& c, float& dc, float (&sum)[4]) {
#pragma unroll
    for (int i = 0; i < SRU_P; ++i) {
        const int s = s0 + i;
        if (FULL || s < T) {
            const float u0 = ru[i][0], u1 = ru[i][1], u2 = ru[i][2], u3 = ru[i][3];
            const float xv = rx[i], cp = rc[i];
            const float dy = ((DYS & 1) ? rdy[i] : 0.0f) + ((DYS & 2) ? rdm[i] * p.mn : 0.0f);
            if (FULL || s + SRU_P < T) {
                const long ea = e + SRU_P * de;
                sru_load_u<K>(U + ea * K, ru[i]);
                if (HASX) rx[i] = x[ea];
                if (FULL || s + SRU_P + 1 < T) rc[i] = C[ea + de];
                else rc[i] = 0.0f;
                if (DYS & 1) rdy[i] = dY[ea];
                if (DYS & 2) rdm[i] = dYm[ea];
            }
            __builtin_amdgcn_sched_barrier(0);
            const float f = sru_sigmoid(u1 + p.vf * cp + p.bf);
            const float r = sru_sigmoid(u2 + p.vr * cp + p.br);
            float g;
            const float ga = sru_act_grad(p.act, c, g);
            const float xp = K == 4 ? u3 : (HASX ? p.scale_x * xv : 0.0f);
            const float du2 = dy * (g * p.m - xp) * r * (1.0f - r);
            const float dxp = dy * (1.0f - r);
            const float dct = dc + dy * r * p.m * ga;
            const float du1 = dct * (cp - u0) * f * (1.0f - f);
            const float du0 = dct * (1.0f - f);
            dc = dct * f + du1 * p.vf + du2 * p.vr;
            sum[0] += du1 * cp, sum[1] += du2 * cp, sum[2] += du1, sum[3] += du2;
            sru_store_u<K>(U + e * K, du0, du1, du2, dxp);
            if (HASX) dxs[e] = dxp * p.scale_x;
            c = cp;
            e += de;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// U is read as U and written as dU (same element, same thread, after its load): no __restrict__ on it.
template <int K, bool HASX, int DYS>
__global__ void __launch_bounds__(SRU_THREADS, 3) pk_sru_bwd_kernel(float* U, const float* __restrict__ C,
                                                                    const float* __restrict__ x, float scale_x,
                                                                    const float* __restrict__ wc, const float* __restrict__ bias,
                                                                    const float* __restrict__ mh, const float* __restrict__ dY,
                                                                    const float* __restrict__ dYm,
                                                                    const float* __restrict__ mnext, int T, int B, int H,
                                                                    int out, int act, float* __restrict__ dxs,
                                                                    float* __restrict__ part) {
    SruCol q;
    if (!sru_col(T, B, H, out, nullptr, q)) return;
    const SruPar p = {wc[q.col], wc[out + q.col], bias[q.col], bias[out + q.col], mh != nullptr ? mh[q.gid] : 1.0f,
                      mnext != nullptr ? mnext[q.gid] : 1.0f, scale_x, act};
    // walk index s: direction 0 walks down from T - 1, direction 1 up from 0 (the reverse of the forward walk)
    long e = q.dir ? q.gid : (long)(T - 1) * q.step + q.gid;
    const long de = q.dir ? q.step : -q.step;

    float ru[SRU_P][4], rx[SRU_P], rc[SRU_P], rdy[SRU_P], rdm[SRU_P];
    float c = C[e], dc = 0.0f, sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < SRU_P; ++i) {  // branch-free: slots behind the last step re-read the last step and are never used
        const long ea = e + (i < T ? i : T - 1) * de;
        sru_load_u<K>(U + ea * K, ru[i]);
        rx[i] = HASX ? x[ea] : 0.0f;
        const float cn = C[e + (i + 1 < T ? i + 1 : T - 1) * de];
        rc[i] = i + 1 < T ? cn : 0.0f;
        rdy[i] = (DYS & 1) ? dY[ea] : 0.0f;
        rdm[i] = (DYS & 2) ? dYm[ea] : 0.0f;
    }
    int s0 = 0;
    for (; s0 + 2 * SRU_P < T; s0 += SRU_P)
        sru_bwd_block<K, HASX, DYS, true>(U, C, x, dY, dYm, dxs, p, e, de, s0, T, ru, rx, rc, rdy, rdm, c, dc, sum);
    for (; s0 < T; s0 += SRU_P)
        sru_bwd_block<K, HASX, DYS, false>(U, C, x, dY, dYm, dxs, p, e, de, s0, T, ru, rx, rc, rdy, rdm, c, dc, sum);
    float* o = part + (q.gid / out) * 4 * (long)out + q.col;
    o[0] = sum[0], o[out] = sum[1], o[2 * (long)out] = sum[2], o[3 * (long)out] = sum[3];
}

template <int K, bool HASX> void sru_bwd_launch(dim3 grid, hipStream_t st, float* U, const float* C, const float* x,
                                                float scale_x, const float* wc, const float* bias, const float* mh,
                                                const float* dY, const float* dYm, const float* mnext, int T, int B, int H,
                                                int out, int act, float* dxs, float* part) {
    const dim3 block(SRU_THREADS);
    if (dY != nullptr && dYm != nullptr)
        hipLaunchKernelGGL((pk_sru_bwd_kernel<K, HASX, 3>), grid, block, 0, st, U, C, x, scale_x, wc, bias, mh, dY, dYm, mnext, T, B, H,
                           out, act, dxs, part);
    else if (dYm != nullptr)
        hipLaunchKernelGGL((pk_sru_bwd_kernel<K, HASX, 2>), grid, block, 0, st, U, C, x, scale_x, wc, bias, mh, dY, dYm, mnext, T, B, H,
                           out, act, dxs, part);
    else
        hipLaunchKernelGGL((pk_sru_bwd_kernel<K, HASX, 1>), grid, block, 0, st, U, C, x, scale_x, wc, bias, mh, dY, dYm, mnext, T, B, H,
                           out, act, dxs, part);
}

// out[t][i] = x[t][i] * mask[i]: the time-constant input mask m_rnn of the FIRST layer (the scan writes the masked copy
// of every inner layer's output itself) and, with the same arguments, its backward.
__global__ void __launch_bounds__(256) pk_sru_mask_kernel(const float* __restrict__ x, const float* __restrict__ mask, long T,
                                                          long n, float* __restrict__ out) {
    const long total = T * n, stride = (long)gridDim.x * blockDim.x;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) out[e] = x[e] * mask[e % n];
}

int sru_check(const char* who, int T, int B, int ndir, int H, int k, int act) {
    PK_REQUIRE(T >= 1 && B >= 1 && H >= 1, "%s: T = %d, B = %d, H = %d must be positive", who, T, B, H);
    PK_REQUIRE(ndir == 1 || ndir == 2, "%s: %d directions (1 or 2)", who, ndir);
    PK_REQUIRE(k == 3 || k == 4, "%s: k = %d matrices per unit (3 or 4)", who, k);
    PK_REQUIRE(act >= PK_SRU_ACT_NONE && act <= PK_SRU_ACT_SELU, "%s: unknown activation code %d", who, act);
    PK_REQUIRE((long)B * ndir * H <= (1L << 31) - 1 - SRU_THREADS, "%s: %d x %d x %d columns are out of range", who, B, ndir, H);
    return 0;
}

}  // namespace

extern "C" int pk_sru_fwd(void* stream, int T, int B, int ndir, int H, int k, int act, const float* U, const float* x,
                          float scale_x, const float* weight_c, const float* bias, const float* mask_h, const int32_t* lens,
                          const float* mask_next, float* Y, float* C, float* Ym) {
    if (int rc = sru_check("pk_sru_fwd", T, B, ndir, H, k, act)) return rc;
    PK_REQUIRE(U != nullptr && weight_c != nullptr && bias != nullptr && Y != nullptr,
               "pk_sru_fwd: U, weight_c, bias or Y are NULL");
    PK_REQUIRE(k == 3 || x == nullptr, "pk_sru_fwd: a skip source with k = 4 (the fourth matrix is the skip term)");
    PK_REQUIRE(k == 3 || (reinterpret_cast<uintptr_t>(U) & 15u) == 0, "pk_sru_fwd: U is not 16-byte aligned");
    PK_REQUIRE(lens == nullptr || C == nullptr, "pk_sru_fwd: sentence lengths are forward only (C must be NULL)");
    PK_REQUIRE(mask_next == nullptr || Ym != nullptr, "pk_sru_fwd: a mask for the masked copy without the copy");
    const int out = ndir * H;
    const dim3 grid((unsigned)(((long)B * out + SRU_THREADS - 1) / SRU_THREADS)), block(SRU_THREADS);
    if (k == 4)
        hipLaunchKernelGGL((pk_sru_fwd_kernel<4, false>), grid, block, 0, pk_stream(stream), U, x, scale_x, weight_c, bias, mask_h,
                           lens, mask_next, T, B, H, out, act, Y, C, Ym);
    else if (x != nullptr)
        hipLaunchKernelGGL((pk_sru_fwd_kernel<3, true>), grid, block, 0, pk_stream(stream), U, x, scale_x, weight_c, bias, mask_h,
                           lens, mask_next, T, B, H, out, act, Y, C, Ym);
    else
        hipLaunchKernelGGL((pk_sru_fwd_kernel<3, false>), grid, block, 0, pk_stream(stream), U, x, scale_x, weight_c, bias, mask_h,
                           lens, mask_next, T, B, H, out, act, Y, C, Ym);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_sru_bwd(void* stream, int T, int B, int ndir, int H, int k, int act, float* U, const float* C, const float* x,
                          float scale_x, const float* weight_c, const float* bias, const float* mask_h, const float* dY,
                          const float* dYm, const float* mask_next, float* dx_skip, float* partial) {
    if (int rc = sru_check("pk_sru_bwd", T, B, ndir, H, k, act)) return rc;
    PK_REQUIRE(U != nullptr && C != nullptr && weight_c != nullptr && bias != nullptr && partial != nullptr,
               "pk_sru_bwd: U, C, weight_c, bias or the partial sums are NULL");
    PK_REQUIRE(dY != nullptr || dYm != nullptr, "pk_sru_bwd: both output gradients are NULL");
    PK_REQUIRE(dYm == nullptr || mask_next != nullptr, "pk_sru_bwd: a gradient of the masked copy without its mask");
    PK_REQUIRE(k == 3 || (x == nullptr && dx_skip == nullptr), "pk_sru_bwd: a skip source with k = 4");
    PK_REQUIRE((x == nullptr) == (dx_skip == nullptr), "pk_sru_bwd: the skip source and its gradient go together");
    PK_REQUIRE(k == 3 || (reinterpret_cast<uintptr_t>(U) & 15u) == 0, "pk_sru_bwd: U is not 16-byte aligned");
    const int out = ndir * H;
    const dim3 grid((unsigned)(((long)B * out + SRU_THREADS - 1) / SRU_THREADS));
    if (k == 4)
        sru_bwd_launch<4, false>(grid, pk_stream(stream), U, C, x, scale_x, weight_c, bias, mask_h, dY, dYm, mask_next, T, B, H, out,
                                 act, dx_skip, partial);
    else if (x != nullptr)
        sru_bwd_launch<3, true>(grid, pk_stream(stream), U, C, x, scale_x, weight_c, bias, mask_h, dY, dYm, mask_next, T, B, H, out,
                                act, dx_skip, partial);
    else
        sru_bwd_launch<3, false>(grid, pk_stream(stream), U, C, x, scale_x, weight_c, bias, mask_h, dY, dYm, mask_next, T, B, H, out,
                                 act, dx_skip, partial);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_sru_mask(void* stream, const float* x, const float* mask, int64_t T, int64_t n, float* out) {
    PK_REQUIRE(T >= 1 && n >= 1 && T <= (1LL << 40) / n, "pk_sru_mask: T = %lld rows of %lld are out of range", (long long)T,
               (long long)n);
    PK_REQUIRE(x != nullptr && mask != nullptr && out != nullptr, "pk_sru_mask: the input, the mask or the output are NULL");
    long blocks = (long)((T * n + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(pk_sru_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, pk_stream(stream), x, mask, (long)T, (long)n, out);
    PK_LAUNCH_CHECK();
    return 0;
}
