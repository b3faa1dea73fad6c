// pk_seqlen.hip - length-aware data movement around the recurrent layers of a decoding batch: B sentences of lengths
// L_b (1 <= L_b <= T), zero-padded at the END.  The reference's bidirectional layers compute cat([x, flip(x)], dim=1) on
// one sentence; in a padded batch a plain time reversal would start a short sentence's backward direction inside the
// padding.  Here the reversal is per sentence, so that every sentence's rows are what it gives on its own:
//
//   pack   out_f[t][b] = x[t][b]              out_r[t][b] = x[L_b-1-t][b]                      t < L_b,  0 behind
//   join   y_f[t][b]   = [hf[t][b], hb[L_b-1-t][b]]         y_r[t][b] = y_f[L_b-1-t][b]        t < L_b,  0 behind
//
// Plain grid-stride kernels, one element (or one 16-byte vector) per thread and trip: nothing is exchanged between
// workgroups, every output element is written exactly once.  The vector form needs widths and pitches that are multiples
// of 4 floats and 16-byte aligned pointers; anything else takes the scalar form.  A length outside 0 .. T is clamped into
// that range by the kernels (the callers check on the host): no index leaves the tensors whatever `lens` holds.
//
// Behind the head, pk_post_normalize subtracts the log-priors from the log-posteriors and drops the padding rows in one
// more streaming pass (described at its kernel below).
#include "pk_common.h"

namespace {

constexpr int PK_SEQLEN_THREADS = 256;
constexpr long PK_SEQLEN_MAX_BLOCKS = 2048;  // 8 workgroups per CU; the stride loop covers the rest

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<4> { typedef f32x4 type; };

template <int V> __device__ __forceinline__ typename Vec<V>::type zero_vec();
template <> __device__ __forceinline__ float zero_vec<1>() { return 0.0f; }
template <> __device__ __forceinline__ f32x4 zero_vec<4>() { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }

__device__ __forceinline__ long clamped_len(const int32_t* __restrict__ lens, long b, long T) {
    const long L = lens[b];
    return L < 0 ? 0 : (L > T ? T : L);
}

// One unit = V floats of an input row [D].  Pitches in units of V floats.
template <int V>
__global__ void __launch_bounds__(PK_SEQLEN_THREADS) seq_pack_len_kernel(const float* __restrict__ x,
                                                                         const int32_t* __restrict__ lens, long T, long B,
                                                                         long dv, float* __restrict__ out_f,
                                                                         float* __restrict__ out_r, long ldov) {
    typedef typename Vec<V>::type vec_t;
    const long n = T * B * dv, stride = (long)gridDim.x * blockDim.x;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const long t = k / (B * dv), rest = k - t * (B * dv);
        const long b = rest / dv, j = rest - b * dv;
        const long L = clamped_len(lens, b, T);
        const long o = t * ldov + b * dv + j;
        if (t < L) {
            if (out_f != nullptr) reinterpret_cast<vec_t*>(out_f)[o] = reinterpret_cast<const vec_t*>(x)[k];
            if (out_r != nullptr)
                reinterpret_cast<vec_t*>(out_r)[o] = reinterpret_cast<const vec_t*>(x)[((L - 1 - t) * B + b) * dv + j];
        } else {
            if (out_f != nullptr) reinterpret_cast<vec_t*>(out_f)[o] = zero_vec<V>();
            if (out_r != nullptr) reinterpret_cast<vec_t*>(out_r)[o] = zero_vec<V>();
        }
    }
}

// One unit = V floats of an output row [2H]; a unit never straddles the two halves (vector form: H % 4 == 0).
template <int V>
__global__ void __launch_bounds__(PK_SEQLEN_THREADS) seq_join_len_kernel(const float* __restrict__ hf,
                                                                         const float* __restrict__ hb, long ldiv,
                                                                         const int32_t* __restrict__ lens, long T, long B,
                                                                         long hv, float* __restrict__ y_f,
                                                                         float* __restrict__ y_r, long ldov) {
    typedef typename Vec<V>::type vec_t;
    const long rowv = 2 * hv, n = T * B * rowv, stride = (long)gridDim.x * blockDim.x;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const long t = k / (B * rowv), rest = k - t * (B * rowv);
        const long b = rest / rowv, j = rest - b * rowv;
        const long L = clamped_len(lens, b, T);
        const long o = b * rowv + j;
        if (t < L) {
            vec_t v;
            if (j < hv) v = reinterpret_cast<const vec_t*>(hf)[t * ldiv + b * hv + j];
            else v = reinterpret_cast<const vec_t*>(hb)[(L - 1 - t) * ldiv + b * hv + (j - hv)];
            if (y_f != nullptr) reinterpret_cast<vec_t*>(y_f)[t * ldov + o] = v;
            if (y_r != nullptr) reinterpret_cast<vec_t*>(y_r)[(L - 1 - t) * ldov + o] = v;
        } else {  // padding: step t of the reversed tensor is padding too
            if (y_f != nullptr) reinterpret_cast<vec_t*>(y_f)[t * ldov + o] = zero_vec<V>();
            if (y_r != nullptr) reinterpret_cast<vec_t*>(y_r)[t * ldov + o] = zero_vec<V>();
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline unsigned blocks_for(long n) {
    long b = (n + PK_SEQLEN_THREADS - 1) / PK_SEQLEN_THREADS;
    if (b < 1) b = 1;
    return (unsigned)(b < PK_SEQLEN_MAX_BLOCKS ? b : PK_SEQLEN_MAX_BLOCKS);
}

// Posterior normalisation of a decoded batch, padding stripped in the same pass:
//   out[i][c] = (T)x[rows ? rows[i] : i][c] - logprior[c]        T = float or double, the type of logprior and out
// The OUTPUT is indexed flat: one unit = 16 bytes of it (V = 4 floats or 2 doubles), which may straddle two rows - C is
// 1938, 48 or 3480 in the recipes, so rows of x are not 16-byte aligned and are read element by element (neighbouring
// lanes read neighbouring addresses).  The last unit may be short.  A row index outside 0 .. R-1 is clamped into that
// range (the caller checks on the host): no index leaves x whatever `rows` holds.  One conversion (exact) and one IEEE
// subtraction per element, nothing to contract.
template <typename T, int V>
__global__ void __launch_bounds__(PK_SEQLEN_THREADS) post_normalize_kernel(const float* __restrict__ x,
                                                                           const int64_t* __restrict__ rows, long R, long C,
                                                                           const T* __restrict__ logprior, long total,
                                                                           T* __restrict__ out) {
    const long units = (total + V - 1) / V, stride = (long)gridDim.x * blockDim.x;
    const bool narrow = total < 0xfffffff0L;  // (a 32-bit division where the flat index allows it)
    for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += stride) {
        const long e0 = u * V;
        long i = narrow ? (long)((unsigned)e0 / (unsigned)C) : e0 / C;
        long c = e0 - i * C;
        T v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (e0 + k < total) {
                long r = rows != nullptr ? (long)rows[i] : i;
                r = r < 0 ? 0 : (r >= R ? R - 1 : r);
                v[k] = (T)x[r * C + c] - logprior[c];
            } else {
                v[k] = (T)0;
            }
            if (++c == C) { c = 0; ++i; }
        }
        if (V > 1 && e0 + V <= total) {
            typedef T vec_t __attribute__((ext_vector_type(V)));
            vec_t w;
#pragma unroll
            for (int k = 0; k < V; ++k) w[k] = v[k];
            *reinterpret_cast<vec_t*>(out + e0) = w;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (e0 + k < total) out[e0 + k] = v[k];
        }
    }
}

template <typename T>
void post_normalize_launch(void* stream, const float* x, const int64_t* rows, long R, long n, long C, const void* logprior,
                           void* out) {
    constexpr int W = 16 / (int)sizeof(T);
    const long total = n * C;
    const dim3 block(PK_SEQLEN_THREADS);
    if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0)
        hipLaunchKernelGGL((post_normalize_kernel<T, W>), dim3(blocks_for((total + W - 1) / W)), block, 0, pk_stream(stream), x, rows, R, C,
                           static_cast<const T*>(logprior), total, static_cast<T*>(out));
    else
        hipLaunchKernelGGL((post_normalize_kernel<T, 1>), dim3(blocks_for(total)), block, 0, pk_stream(stream), x, rows, R, C,
                           static_cast<const T*>(logprior), total, static_cast<T*>(out));
}

}  // namespace

extern "C" int pk_seq_pack_len(void* stream, const float* x, const int32_t* lens, int64_t T, int64_t B, int64_t D, float* out_f,
                               float* out_r, int64_t ldo) {
    PK_REQUIRE(T >= 1 && B >= 1 && D >= 1, "pk_seq_pack_len: T = %lld, B = %lld, D = %lld must be positive", (long long)T,
               (long long)B, (long long)D);
    PK_REQUIRE(x != nullptr && lens != nullptr, "pk_seq_pack_len: the input or the lengths are NULL");
    PK_REQUIRE(out_f != nullptr || out_r != nullptr, "pk_seq_pack_len: both outputs are NULL");
    PK_REQUIRE(B <= (1LL << 40) / D && ldo >= B * D, "pk_seq_pack_len: a pitch of %lld floats is smaller than a step of %lld x %lld",
               (long long)ldo, (long long)B, (long long)D);
    PK_REQUIRE(T <= (1LL << 40) / ldo, "pk_seq_pack_len: [%lld] steps at a pitch of %lld are out of range", (long long)T, (long long)ldo);
    const bool vec = D % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(out_f) && aligned16(out_r);
    const long v = vec ? 4 : 1, n = (long)T * B * D / v;
    const dim3 grid(blocks_for(n)), block(PK_SEQLEN_THREADS);
    if (vec)
        hipLaunchKernelGGL(seq_pack_len_kernel<4>, grid, block, 0, pk_stream(stream), x, lens, (long)T, (long)B, (long)D / 4, out_f, out_r, (long)ldo / 4);
    else
        hipLaunchKernelGGL(seq_pack_len_kernel<1>, grid, block, 0, pk_stream(stream), x, lens, (long)T, (long)B, (long)D, out_f, out_r, (long)ldo);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_seq_join_len(void* stream, const float* hf, const float* hb, int64_t ldi, const int32_t* lens, int64_t T,
                               int64_t B, int64_t H, float* y_f, float* y_r, int64_t ldo) {
    PK_REQUIRE(T >= 1 && B >= 1 && H >= 1, "pk_seq_join_len: T = %lld, B = %lld, H = %lld must be positive", (long long)T,
               (long long)B, (long long)H);
    PK_REQUIRE(hf != nullptr && hb != nullptr && lens != nullptr, "pk_seq_join_len: a direction or the lengths are NULL");
    PK_REQUIRE(y_f != nullptr || y_r != nullptr, "pk_seq_join_len: both outputs are NULL");
    PK_REQUIRE(B <= (1LL << 39) / H && ldi >= B * H, "pk_seq_join_len: an input pitch of %lld floats is smaller than a step of %lld x %lld",
               (long long)ldi, (long long)B, (long long)H);
    PK_REQUIRE(ldo >= 2 * B * H, "pk_seq_join_len: an output pitch of %lld floats is smaller than a step of %lld x %lld",
               (long long)ldo, (long long)B, (long long)(2 * H));
    PK_REQUIRE(T <= (1LL << 40) / ldo && T <= (1LL << 40) / ldi, "pk_seq_join_len: [%lld] steps at pitches of %lld and %lld are out of range",
               (long long)T, (long long)ldi, (long long)ldo);
    const bool vec = H % 4 == 0 && ldi % 4 == 0 && ldo % 4 == 0 && aligned16(hf) && aligned16(hb) && aligned16(y_f) && aligned16(y_r);
    const long v = vec ? 4 : 1, n = (long)T * B * 2 * H / v;
    const dim3 grid(blocks_for(n)), block(PK_SEQLEN_THREADS);
    if (vec)
        hipLaunchKernelGGL(seq_join_len_kernel<4>, grid, block, 0, pk_stream(stream), hf, hb, (long)ldi / 4, lens, (long)T, (long)B, (long)H / 4, y_f, y_r, (long)ldo / 4);
    else
        hipLaunchKernelGGL(seq_join_len_kernel<1>, grid, block, 0, pk_stream(stream), hf, hb, (long)ldi, lens, (long)T, (long)B, (long)H, y_f, y_r, (long)ldo);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_post_normalize(void* stream, const float* x, const int64_t* rows, int64_t R, int64_t n, int64_t C,
                                 const void* logprior, void* out, int f64) {
    PK_REQUIRE(R >= 1 && n >= 1 && C >= 1, "pk_post_normalize: R = %lld, n = %lld, C = %lld must be positive", (long long)R,
               (long long)n, (long long)C);
    PK_REQUIRE(x != nullptr && logprior != nullptr && out != nullptr, "pk_post_normalize: the input, the log-priors or the output are NULL");
    PK_REQUIRE(rows != nullptr || n == R, "pk_post_normalize: without a row map the output has the input's %lld rows, not %lld",
               (long long)R, (long long)n);
    PK_REQUIRE(R <= (1LL << 40) / C && n <= (1LL << 40) / C, "pk_post_normalize: [%lld] and [%lld] rows of %lld are out of range",
               (long long)R, (long long)n, (long long)C);
    PK_REQUIRE((reinterpret_cast<uintptr_t>(out) & (f64 ? 7u : 3u)) == 0 && (reinterpret_cast<uintptr_t>(logprior) & (f64 ? 7u : 3u)) == 0,
               "pk_post_normalize: the log-priors or the output are not aligned to their element size");
    if (f64) post_normalize_launch<double>(stream, x, rows, (long)R, (long)n, (long)C, logprior, out);
    else post_normalize_launch<float>(stream, x, rows, (long)R, (long)n, (long)C, logprior, out);
    PK_LAUNCH_CHECK();
    return 0;
}
