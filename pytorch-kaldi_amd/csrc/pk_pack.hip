// pk_pack.hip - the data movement around torch-layout (nn.LSTM / nn.RNN) recurrent layers that run on the engine's cells
// (neural_networks.py:153-203, :256-297): gate blocks re-ordered between torch's packing and the kernels', the two biases
// summed, and the join of a layer's two directions with time reversal and inter-layer dropout.
//
//   pack     Wcat[g*H + r][:] = w_ih[perm[g]*H + r][:]      Ucat likewise      bcat[g*H + r] = b_ih[..] + b_hh[..]
//   unpack   dw_ih[perm[g]*H + r][:] = dWcat[g*H + r][:]    dw_hh likewise     db_ih[..] = db_hh[..] = dbcat[g*H + r]
//   join     y[t][b][0:H] = yf[t][b][:] * scale,  y[t][b][H:2H] = yb[T-1-t][b][:] * scale, zero where the mask is 0;
//            y_rev[t] = y[T-1-t];  backward is the transpose
//
// Plain grid-stride kernels, one element (or one 16-byte vector) per thread and trip: nothing is exchanged between
// workgroups.  Every element is read once and written once (twice when both y and y_rev are asked for).  The vector form
// needs row lengths that are multiples of 4 floats and 16-byte aligned pointers; anything else takes the scalar form.
#include "pk_common.h"

namespace {

constexpr int PK_PACK_THREADS = 256;
constexpr long PK_PACK_MAX_BLOCKS = 2048;  // 8 workgroups per CU; the stride loop covers the rest

struct GatePerm {
    int p[PK_PACK_MAX_GATES];
};

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<4> { typedef f32x4 type; };

// Rows of length `cols` (in units of V floats) move from block sb[g] of src to block db[g] of dst, r inside a block kept.
template <int V>
__device__ __forceinline__ void move_blocks(const float* __restrict__ src, float* __restrict__ dst, long H, long cols, int G,
                                            const GatePerm& perm, int inverse, long first, long stride) {
    typedef typename Vec<V>::type vec_t;
    const long cv = cols / V, per_gate = H * cv, n = (long)G * per_gate;
    for (long k = first; k < n; k += stride) {
        const int g = (int)(k / per_gate);
        const long rest = k - (long)g * per_gate;
        const long sb = inverse ? g : perm.p[g], db = inverse ? perm.p[g] : g;
        reinterpret_cast<vec_t*>(dst)[db * per_gate + rest] = reinterpret_cast<const vec_t*>(src)[sb * per_gate + rest];
    }
}

// inverse = 0 (pack): w0 / u0 -> w1 / u1, bo0 = ba + bb (a NULL one counts as 0).
// inverse = 1 (unpack): the same with source and destination blocks swapped, ba -> bo0 and bo1.
template <int V>
__global__ void __launch_bounds__(PK_PACK_THREADS) gates_move_kernel(const float* __restrict__ w0, float* __restrict__ w1, int D,
                                                                     const float* __restrict__ u0, float* __restrict__ u1,
                                                                     const float* __restrict__ ba, const float* __restrict__ bb,
                                                                     float* __restrict__ bo0, float* __restrict__ bo1, int G,
                                                                     int H, GatePerm perm, int inverse) {
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    if (w0 != nullptr) move_blocks<V>(w0, w1, H, D, G, perm, inverse, first, stride);
    if (u0 != nullptr) move_blocks<V>(u0, u1, H, H, G, perm, inverse, first, stride);
    if (bo0 == nullptr && bo1 == nullptr) return;
    for (long k = first; k < (long)G * H; k += stride) {
        const int g = (int)(k / H);
        const long r = k - (long)g * H;
        const long s = (inverse ? g : perm.p[g]) * (long)H + r, d = (inverse ? perm.p[g] : g) * (long)H + r;
        float v;
        if (ba != nullptr && bb != nullptr) v = ba[s] + bb[s];
        else v = ba != nullptr ? ba[s] : bb[s];
        if (bo0 != nullptr) bo0[d] = v;
        if (bo1 != nullptr) bo1[d] = v;
    }
}

__device__ __forceinline__ float keep(float v, float m) { return m != 0.0f ? v : 0.0f; }
__device__ __forceinline__ f32x4 keep(f32x4 v, f32x4 m) {
    return f32x4{keep(v[0], m[0]), keep(v[1], m[1]), keep(v[2], m[2]), keep(v[3], m[3])};
}

// One unit = V floats of an output row [ndir*H]; a unit never straddles the two halves (vector form: H % 4 == 0).
template <int V>
__global__ void __launch_bounds__(PK_PACK_THREADS) seq_join_fwd_kernel(const float* __restrict__ yf, const float* __restrict__ yb,
                                                                       const float* __restrict__ mask, float scale, long T, long B,
                                                                       long H, int ndir, float* __restrict__ y,
                                                                       float* __restrict__ y_rev) {
    typedef typename Vec<V>::type vec_t;
    const long hv = H / V, rowv = ndir * hv, n = T * B * rowv;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const long t = k / (B * rowv), rest = k - t * (B * rowv);
        const long b = rest / rowv, j = rest - b * rowv;
        vec_t v;
        if (j < hv) v = reinterpret_cast<const vec_t*>(yf)[(t * B + b) * hv + j];
        else v = reinterpret_cast<const vec_t*>(yb)[((T - 1 - t) * B + b) * hv + (j - hv)];
        v = v * scale;
        if (mask != nullptr) v = keep(v, reinterpret_cast<const vec_t*>(mask)[k]);
        if (y != nullptr) reinterpret_cast<vec_t*>(y)[k] = v;
        if (y_rev != nullptr) reinterpret_cast<vec_t*>(y_rev)[((T - 1 - t) * B + b) * rowv + j] = v;
    }
}

template <int V>
__global__ void __launch_bounds__(PK_PACK_THREADS) seq_join_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dy_rev,
                                                                       const float* __restrict__ mask, float scale, long T, long B,
                                                                       long H, int ndir, float* __restrict__ dyf,
                                                                       float* __restrict__ dyb) {
    typedef typename Vec<V>::type vec_t;
    const long hv = H / V, rowv = ndir * hv, n = T * B * rowv;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const long t = k / (B * rowv), rest = k - t * (B * rowv);
        const long b = rest / rowv, j = rest - b * rowv;
        const long krev = ((T - 1 - t) * B + b) * rowv + j;
        vec_t g;
        if (dy != nullptr && dy_rev != nullptr)
            g = reinterpret_cast<const vec_t*>(dy)[k] + reinterpret_cast<const vec_t*>(dy_rev)[krev];
        else
            g = dy != nullptr ? reinterpret_cast<const vec_t*>(dy)[k] : reinterpret_cast<const vec_t*>(dy_rev)[krev];
        g = g * scale;
        if (mask != nullptr) g = keep(g, reinterpret_cast<const vec_t*>(mask)[k]);
        if (j < hv) reinterpret_cast<vec_t*>(dyf)[(t * B + b) * hv + j] = g;
        else reinterpret_cast<vec_t*>(dyb)[((T - 1 - t) * B + b) * hv + (j - hv)] = g;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline unsigned blocks_for(long n) {
    long b = (n + PK_PACK_THREADS - 1) / PK_PACK_THREADS;
    if (b < 1) b = 1;
    return (unsigned)(b < PK_PACK_MAX_BLOCKS ? b : PK_PACK_MAX_BLOCKS);
}

int gates_move(const char* who, void* stream, const float* w0, float* w1, const float* u0, float* u1, const float* ba,
               const float* bb, float* bo0, float* bo1, int G, int H, int D, const int* perm, int inverse) {
    PK_REQUIRE(G >= 1 && G <= PK_PACK_MAX_GATES, "%s: G = %d gates (1 .. %d)", who, G, PK_PACK_MAX_GATES);
    PK_REQUIRE(H >= 1 && D >= 1 && H <= (1 << 20) && D <= (1 << 20), "%s: H = %d, D = %d must be positive (up to 2^20)", who, H, D);
    PK_REQUIRE(perm != nullptr, "%s: the gate permutation is NULL", who);
    PK_REQUIRE((w0 == nullptr) == (w1 == nullptr), "%s: the input matrix and its destination go together", who);
    PK_REQUIRE((u0 == nullptr) == (u1 == nullptr), "%s: the recurrent matrix and its destination go together", who);
    if (ba == nullptr && bb == nullptr) bo0 = bo1 = nullptr;  // no bias: the destinations are left as they are
    if (bo0 == nullptr && bo1 == nullptr) ba = bb = nullptr;
    PK_REQUIRE(w0 != nullptr || u0 != nullptr || ba != nullptr || bb != nullptr, "%s: nothing to move", who);
    GatePerm gp = {};
    unsigned seen = 0;
    for (int g = 0; g < G; ++g) {
        PK_REQUIRE(perm[g] >= 0 && perm[g] < G && !((seen >> perm[g]) & 1u), "%s: perm is not a permutation of 0 .. %d", who, G - 1);
        seen |= 1u << perm[g];
        gp.p[g] = perm[g];
    }
    const bool vec = D % 4 == 0 && H % 4 == 0 && aligned16(w0) && aligned16(w1) && aligned16(u0) && aligned16(u1);
    const long rows = (long)G * H, v = vec ? 4 : 1;
    long n = (ba != nullptr || bb != nullptr) ? rows : 0;
    if (w0 != nullptr && rows * D / v > n) n = rows * D / v;
    if (u0 != nullptr && rows * H / v > n) n = rows * H / v;
    const dim3 grid(blocks_for(n)), block(PK_PACK_THREADS);
    if (vec)
        hipLaunchKernelGGL(gates_move_kernel<4>, grid, block, 0, pk_stream(stream), w0, w1, D, u0, u1, ba, bb, bo0, bo1, G, H, gp, inverse);
    else
        hipLaunchKernelGGL(gates_move_kernel<1>, grid, block, 0, pk_stream(stream), w0, w1, D, u0, u1, ba, bb, bo0, bo1, G, H, gp, inverse);
    PK_LAUNCH_CHECK();
    return 0;
}

int join_check(const char* who, int64_t T, int64_t B, int64_t H, int ndir, const void* half0, const void* half1, const void* full0,
               const void* full1) {
    PK_REQUIRE(T >= 1 && B >= 1 && H >= 1, "%s: T = %lld, B = %lld, H = %lld must be positive", who, (long long)T, (long long)B, (long long)H);
    PK_REQUIRE(ndir == 1 || ndir == 2, "%s: ndir = %d (1 or 2)", who, ndir);
    PK_REQUIRE(T <= (1LL << 40) / B / H / ndir, "%s: [%lld, %lld, %d x %lld] is out of range", who, (long long)T, (long long)B, ndir, (long long)H);
    PK_REQUIRE(half0 != nullptr, "%s: the forward-direction tensor is NULL", who);
    PK_REQUIRE((half1 != nullptr) == (ndir == 2), "%s: the backward-direction tensor goes with ndir = 2 and only with it", who);
    PK_REQUIRE(full0 != nullptr || full1 != nullptr, "%s: both joined tensors are NULL", who);
    return 0;
}

}  // namespace

extern "C" int pk_gates_pack(void* stream, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int G, int H,
                             int D, const int* perm, float* Wcat, float* Ucat, float* bcat) {
    return gates_move("pk_gates_pack", stream, w_ih, Wcat, w_hh, Ucat, b_ih, b_hh, bcat, nullptr, G, H, D, perm, 0);
}

extern "C" int pk_gates_unpack(void* stream, const float* dWcat, const float* dUcat, const float* dbcat, int G, int H, int D,
                               const int* perm, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh) {
    return gates_move("pk_gates_unpack", stream, dWcat, dw_ih, dUcat, dw_hh, dbcat, nullptr, db_ih, db_hh, G, H, D, perm, 1);
}

extern "C" int pk_seq_join_fwd(void* stream, const float* yf, const float* yb, const float* mask, float scale, int64_t T, int64_t B,
                               int64_t H, int ndir, float* y, float* y_rev) {
    if (int rc = join_check("pk_seq_join_fwd", T, B, H, ndir, yf, yb, y, y_rev)) return rc;
    const bool vec = H % 4 == 0 && aligned16(yf) && aligned16(yb) && aligned16(mask) && aligned16(y) && aligned16(y_rev);
    const long n = (long)T * B * ndir * H / (vec ? 4 : 1);
    const dim3 grid(blocks_for(n)), block(PK_PACK_THREADS);
    if (vec)
        hipLaunchKernelGGL(seq_join_fwd_kernel<4>, grid, block, 0, pk_stream(stream), yf, yb, mask, scale, (long)T, (long)B, (long)H, ndir, y, y_rev);
    else
        hipLaunchKernelGGL(seq_join_fwd_kernel<1>, grid, block, 0, pk_stream(stream), yf, yb, mask, scale, (long)T, (long)B, (long)H, ndir, y, y_rev);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_seq_join_bwd(void* stream, const float* dy, const float* dy_rev, const float* mask, float scale, int64_t T,
                               int64_t B, int64_t H, int ndir, float* dyf, float* dyb) {
    if (int rc = join_check("pk_seq_join_bwd", T, B, H, ndir, dyf, dyb, dy, dy_rev)) return rc;
    const bool vec = H % 4 == 0 && aligned16(dy) && aligned16(dy_rev) && aligned16(mask) && aligned16(dyf) && aligned16(dyb);
    const long n = (long)T * B * ndir * H / (vec ? 4 : 1);
    const dim3 grid(blocks_for(n)), block(PK_PACK_THREADS);
    if (vec)
        hipLaunchKernelGGL(seq_join_bwd_kernel<4>, grid, block, 0, pk_stream(stream), dy, dy_rev, mask, scale, (long)T, (long)B, (long)H, ndir, dyf, dyb);
    else
        hipLaunchKernelGGL(seq_join_bwd_kernel<1>, grid, block, 0, pk_stream(stream), dy, dy_rev, mask, scale, (long)T, (long)B, (long)H, ndir, dyf, dyb);
    PK_LAUNCH_CHECK();
    return 0;
}
