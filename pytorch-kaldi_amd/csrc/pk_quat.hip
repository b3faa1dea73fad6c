// pk_quat.hip - quaternion weight matrices (quaternion_neural_networks.py:378-392): the real matrix a quaternion linear
// layer multiplies with, assembled from its four components in the orientation the recurrence and GEMM kernels take
// (nn.Linear's: [out, in], gates stacked row-wise), and the fold of that matrix' gradient back onto the components.
//
//   W[g*4O + q*O + o, p*I + i] = S[q][p] * comp[g][q ^ p][i][o]        q, p in 0..3 (output / input block), r,i,j,k = 0..3
//
// The component index of block (q, p) is q ^ p; S is the sign table of the Hamilton product below.  A component is
// [I][O] with o contiguous, W has i contiguous: both kernels move 32 x 32 tiles through LDS (rows padded to 33 floats: the
// transposed read walks a column, 33 is odd, so the 32 lanes of a half wave hit 32 banks) so that global loads and stores
// are both along the contiguous index.  A component element is read once and written to its four blocks; the fold reads
// the four blocks and sums them pairwise, (t0 + t1) + (t2 + t3), then adds the previous value when beta = 1: every term
// passes through at most three roundings.  Memory bound: 20 B per component element each way.
#include "pk_common.h"

namespace {

constexpr int QT = 32;       // tile edge
constexpr int QROWS = 8;     // blockDim.y: a thread covers QT / QROWS rows of the tile

struct QuatPtrs {
    const float* p[4 * PK_QUAT_MAX_GATES];
};
struct QuatPtrsOut {
    float* p[4 * PK_QUAT_MAX_GATES];
};

__device__ __forceinline__ float quat_sign(int q, int p) {
    // rows: output block q; columns: input block p
    //   r:  + - - -      i:  + + - +      j:  + + + -      k:  + - + +
    constexpr unsigned minus = 0x0Eu | (0x04u << 4) | (0x08u << 8) | (0x02u << 12);
    return ((minus >> (4 * q + p)) & 1u) ? -1.0f : 1.0f;
}

// grid (ceil(O / 32), ceil(I / 32), 4 G), block (32, 8)
__global__ void __launch_bounds__(QT* QROWS) quat_assemble_kernel(QuatPtrs tab, const float* __restrict__ base, int I, int O,
                                                                  float* __restrict__ W) {
    __shared__ float tile[QT][QT + 1];
    const int gc = blockIdx.z, g = gc >> 2, c = gc & 3;
    const long IO = (long)I * O;
    const float* __restrict__ src = base != nullptr ? base + gc * IO : tab.p[gc];
    const int i0 = blockIdx.y * QT, o0 = blockIdx.x * QT;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < QT; r += QROWS) {  // rows i, lanes along o
        const int i = i0 + r, o = o0 + tx;
        tile[r][tx] = (i < I && o < O) ? src[(long)i * O + o] : 0.0f;
    }
    __syncthreads();
    const long ldw = 4L * I;
    const int i = i0 + tx;
    if (i >= I) return;
    for (int r = ty; r < QT; r += QROWS) {  // rows o, lanes along i
        const int o = o0 + r;
        if (o >= O) break;
        const float v = tile[tx][r];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = q ^ c;
            W[((long)g * 4 * O + (long)q * O + o) * ldw + (long)p * I + i] = quat_sign(q, p) * v;
        }
    }
}

// same grid; dcomp[g][c][i][o] = sum_q S[q][q^c] dW[g*4O + q*O + o, (q^c)*I + i]  (+ the previous value when accumulate)
__global__ void __launch_bounds__(QT* QROWS) quat_fold_kernel(const float* __restrict__ dW, int I, int O, int accumulate,
                                                              QuatPtrsOut tab, float* __restrict__ base) {
    __shared__ float tile[4][QT][QT + 1];
    const int gc = blockIdx.z, g = gc >> 2, c = gc & 3;
    const long IO = (long)I * O;
    float* __restrict__ dst = base != nullptr ? base + gc * IO : tab.p[gc];
    const int i0 = blockIdx.y * QT, o0 = blockIdx.x * QT;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long ldw = 4L * I;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = q ^ c;
        const float s = quat_sign(q, p);
        for (int r = ty; r < QT; r += QROWS) {  // rows o, lanes along i
            const int o = o0 + r, i = i0 + tx;
            tile[q][r][tx] = (i < I && o < O) ? s * dW[((long)g * 4 * O + (long)q * O + o) * ldw + (long)p * I + i] : 0.0f;
        }
    }
    __syncthreads();
    const int o = o0 + tx;
    if (o >= O) return;
    for (int r = ty; r < QT; r += QROWS) {  // rows i, lanes along o
        const int i = i0 + r;
        if (i >= I) break;
        float v = (tile[0][tx][r] + tile[1][tx][r]) + (tile[2][tx][r] + tile[3][tx][r]);
        const long at = (long)i * O + o;
        if (accumulate) v += dst[at];
        dst[at] = v;
    }
}

int quat_check(const char* who, const void* table, const void* base, int G, int I, int O, const void* mat) {
    PK_REQUIRE(mat != nullptr, "%s: the matrix pointer is NULL", who);
    PK_REQUIRE((table != nullptr) != (base != nullptr), "%s: exactly one of the pointer table and the base pointer must be given", who);
    PK_REQUIRE(G >= 1 && G <= PK_QUAT_MAX_GATES, "%s: G = %d gates (1 .. %d)", who, G, PK_QUAT_MAX_GATES);
    PK_REQUIRE(I >= 1 && O >= 1, "%s: component shape [%d, %d] must be positive", who, I, O);
    // (grid.y = ceil(I / 32) <= 65535)
    PK_REQUIRE(I <= (1 << 20) && O <= (1 << 24), "%s: component shape [%d, %d] is out of range", who, I, O);
    return 0;
}

}  // namespace

extern "C" int pk_quat_assemble(void* stream, const float* const* comps, const float* base, int G, int I, int O, float* W) {
    if (int rc = quat_check("pk_quat_assemble", comps, base, G, I, O, W)) return rc;
    QuatPtrs tab = {};
    if (comps != nullptr) {
        for (int k = 0; k < 4 * G; ++k) {
            PK_REQUIRE(comps[k] != nullptr, "pk_quat_assemble: component %d of the pointer table is NULL", k);
            tab.p[k] = comps[k];
        }
    }
    const dim3 grid((O + QT - 1) / QT, (I + QT - 1) / QT, 4 * G), block(QT, QROWS);
    hipLaunchKernelGGL(quat_assemble_kernel, grid, block, 0, pk_stream(stream), tab, base, I, O, W);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_quat_fold(void* stream, const float* dW, int G, int I, int O, float beta, float* const* dcomps, float* dbase) {
    if (int rc = quat_check("pk_quat_fold", dcomps, dbase, G, I, O, dW)) return rc;
    PK_REQUIRE(beta == 0.0f || beta == 1.0f, "pk_quat_fold: beta = %g (0 overwrites, 1 accumulates)", (double)beta);
    QuatPtrsOut tab = {};
    if (dcomps != nullptr) {
        for (int k = 0; k < 4 * G; ++k) {
            PK_REQUIRE(dcomps[k] != nullptr, "pk_quat_fold: component %d of the pointer table is NULL", k);
            tab.p[k] = dcomps[k];
        }
    }
    const dim3 grid((O + QT - 1) / QT, (I + QT - 1) / QT, 4 * G), block(QT, QROWS);
    hipLaunchKernelGGL(quat_fold_kernel, grid, block, 0, pk_stream(stream), dW, I, O, beta != 0.0f ? 1 : 0, tab, dbase);
    PK_LAUNCH_CHECK();
    return 0;
}
