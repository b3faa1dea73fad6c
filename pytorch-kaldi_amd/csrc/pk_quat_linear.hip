// pk_quat_linear.hip - the quaternion linear layer (quaternion_neural_networks.py:378-477: quaternion_linear and
// QuaternionLinearFunction) without the real matrix it stands for (include/pk_amd.h: pk_quat_linear_*).
//
//     Y[n][q*O + o]   = bias[q*O + o] + sum_p S[q][p] * sum_i X[n][p*I + i] * comp[q^p][i][o]
//     dX[n][p*I + i]  =                 sum_q S[q][p] * sum_o dY[n][q*O + o] * comp[q^p][i][o]
//     dcomp[c][i][o]  = beta*dcomp[c][i][o] + sum_q S[q][q^c] * sum_n X[n][(q^c)*I + i] * dY[n][q*O + o]
//     dbias[q*O + o]  = sum_n dY[n][q*O + o]
//
// All three are ONE pattern.  Two operands come in four blocks each, A[x] (rows r, reduction index k) and B[y] (rows w,
// reduction index k), and the 16 block products land in four accumulator sets, acc[x ^ y] += +-A[x] . B[y]^T:
//
//     forward   A[x] = X block p = x    [n][i]    B[y] = comp y  as [o][i]    acc[q = x^y]   sign S[x^y][x]
//     dX        A[x] = dY block q = x   [n][o]    B[y] = comp y  as [i][o]    acc[p = x^y]   sign S[x][x^y]
//     dcomp     A[x] = X block p = x    [i][n]    B[y] = dY block q = y [o][n] acc[c = x^y]   sign S[y][x]
//
// Work split.  A workgroup (four waves, 2 x 2) owns TM = 32 * RT rows of A by 32 rows of B and all four accumulator sets
// of that tile; a wave owns RT 16 x 16 MFMA tiles of each set (RT = 2 where the grid still fills the device, else 1).
// Per step of 32 along k it stages the four A tiles and the four B tiles in LDS ONCE and issues the 16 signed products
// from them: every fragment a lane reads from LDS feeds four matrix instructions (an A fragment the four B blocks, a B
// fragment the four A blocks of each row tile), 8 reads for 16 MFMAs at RT = 1, 12 for 32 at RT = 2.  The sign is a flip of
// the sign bit of the A fragment in registers (one v_xor per fragment; four per 8-wide bf16 fragment), chosen at compile
// time per (x, y): no negated copy of anything goes to LDS or HBM and the dense [4O][4I] matrix never exists.
//
// LDS layout.  Both operands lie as [block][row][k] with k contiguous, whatever their layout in memory, so that the
// fragment reads are the same in all three kernels.  fp32 rows are padded to 34 floats: an MFMA operand fragment is
// (row lr, k = lq) for lane 16*lq + lr, a half wave reads 16 rows x 2 k, and 34*lr + lq covers 32 different banks (an
// unpadded 32 would put all 16 rows on one).  bf16 rows are padded to 40 elements: a lane reads the 8 consecutive k of
// v_mfma_f32_16x16x32_bf16 as one 16-byte word, 80-byte rows keep those aligned and spread over the banks.
// Global loads always run along the index that is contiguous in memory - k for X / dY as A and for a component in dX,
// the row index for a component in forward (o) and for X / dY in dcomp (i, o) - as 16-byte loads where base, pitch and
// extent allow (I resp. O a multiple of 4, 16-byte aligned bases), else as 4-byte loads; in the second case the tile is
// transposed by the LDS write (4-byte or 2-byte stores down a column of the padded tile).  Ragged tiles are zero-filled
// on load in all three dimensions and masked on store.
//
// dcomp / dbias.  The reduction index is the row n; the rows are split into slices over gridDim.z so that the grid fills
// the device (about 1024 workgroups, slices of at least 256 rows).  Each workgroup writes its four accumulator sets to
// workspace[slice]; the workgroups of the first i-tile also add up, in fp32 and BEFORE any rounding to bf16, the dY
// values they stage anyway (per thread over its rows, then over the threads of a column in a fixed order through LDS)
// and write them to the bias part of workspace[slice].  A second small kernel adds the slices in ascending order and
// applies beta: bit-identical from run to run, no atomics, no workgroup waits for another.  The dense weight gradient
// and its fold do not exist.
//
// Precision.  PK_PREC_F32: v_mfma_f32_16x16x4_f32, exact fp32 products.  PK_PREC_BF16: operands rounded to bf16 (round to
// nearest even, pk_f2bf - the rounding of the bf16 GEMM's staging) on their way into LDS, v_mfma_f32_16x16x32_bf16, fp32
// accumulation.  No software pipelining across k steps in this family: the loads of a step are hidden by the other
// workgroups of the CU (26 .. 52 KB of LDS each).
//
// Two families.  The one described so far (variant 0) serves calls with few rows.  The wide family further down (variant 1:
// 128 x 64 block pairs, two LDS stages, the loads of step k + 1 in flight under the MFMAs of step k) serves sequence-sized
// batches; ql_variant() holds the measured rule that picks one per (pass, precision, shape), pk_quat_linear_set_variant
// forces either.  Both take the same QlArgs and sign masks and give the same sums in a different order.
#include "pk_common.h"

namespace {

constexpr int QL_KC = 32;       // k per step
constexpr int QL_TW = 32;       // rows of B per workgroup
constexpr int QL_THREADS = 256;
constexpr int QL_PF = QL_KC + 2;  // LDS row pitch, fp32 (floats)
constexpr int QL_PB = QL_KC + 8;  // LDS row pitch, bf16 (elements)
constexpr int QL_FWD = 0, QL_DX = 1, QL_DW = 2;
constexpr int QL_MAX_SLICES = 1024, QL_MIN_SLICE = 256, QL_FILL = 1024;
constexpr int QL_FILL_RT2 = 256;  // forward / dX: 64-row tiles once they give every CU of an MI355X a workgroup

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// S[q][p] < 0: bit 4*q + p (the table of pk_quat.hip)
//   r:  + - - -      i:  + + - +      j:  + + + -      k:  + - + +
constexpr unsigned QL_MINUS = 0x0Eu | (0x04u << 4) | (0x08u << 8) | (0x02u << 12);
// bit 4*x + y: the product A[x] . B[y] enters acc[x ^ y] negated
constexpr unsigned ql_flips(int mode) {
    unsigned m = 0;
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {
            const int q = mode == QL_FWD ? (x ^ y) : mode == QL_DX ? x : y;
            const int p = mode == QL_FWD ? x : mode == QL_DX ? (x ^ y) : x;
            if ((QL_MINUS >> (4 * q + p)) & 1u) m |= 1u << (4 * x + y);
        }
    return m;
}

struct QlOp {
    const float* p[4];  // the four blocks
    long ld;            // pitch of the index that is NOT contiguous
    long rmax;          // extent of the row index
    int vec;            // 16-byte loads
};
struct QlArgs {
    QlOp a, b;
    long kw;            // extent of the reduction index
    long rows;          // dcomp: rows per slice
    float* out;         // Y / dX [n][ldo], or the workspace
    long ldo, outw;     // forward / dX: pitch and block width of out;  dcomp: I*O and O
    const float* bias;  // forward, or NULL
    float* pbias;       // dcomp: bias part of the workspace, or NULL
};
struct QlPtrsOut {
    float* p[4];
};

template <bool BF>
__device__ __forceinline__ void ql_put(void* lds, int at, float v) {
    if (BF) reinterpret_cast<unsigned short*>(lds)[at] = pk_f2bf(v);
    else reinterpret_cast<float*>(lds)[at] = v;
}

// Stage the four [R][32] tiles of one operand: element (blk, r, k) = op.p[blk][(r0 + r) * ld + k0 + k] (KCONT) or
// op.p[blk][(k0 + k) * ld + r0 + r] (row index contiguous), zero outside rmax / kend.  SUM (dcomp's dY, R = 32): the
// thread also adds what it loads into bsum[blk][e]; its column(s) are the same in every step (256 % 8 == 256 % 32 == 0).
template <bool KCONT, bool BF, int R, bool SUM>
__device__ __forceinline__ void ql_stage(void* lds, const QlOp& op, long r0, long k0, long kend, float (&bsum)[4][4]) {
    constexpr int P = BF ? QL_PB : QL_PF;
    const int tid = threadIdx.x;
    if (op.vec) {
        constexpr int C4 = (KCONT ? QL_KC : R) / 4, NC = KCONT ? R : QL_KC, PER = NC * C4 / QL_THREADS;
        static_assert(NC * C4 % QL_THREADS == 0, "a block is a whole number of passes");
#pragma unroll
        for (int j = 0; j < 4 * PER; ++j) {
            const int blk = j / PER, idx = tid + (j % PER) * QL_THREADS;
            const int c4 = idx % C4, run = idx / C4;
            const int r = KCONT ? run : 4 * c4, k = KCONT ? 4 * c4 : run;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < op.rmax && k0 + k < kend)  // (the contiguous extent is a multiple of 4: all four or none)
                v = *reinterpret_cast<const f32x4*>(op.p[blk] + (KCONT ? (r0 + r) * op.ld + k0 + k : (k0 + k) * op.ld + r0 + r));
            if (SUM) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bsum[blk][e] += v[e];
            }
            const int at = (blk * R + r) * P + k;
            if (KCONT) {
                if (BF) {
                    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(lds) + at) = make_uint2(pk_pack_bf2(v[0], v[1]), pk_pack_bf2(v[2], v[3]));
                } else {
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(lds) + at) = make_float2(v[0], v[1]);
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(lds) + at + 2) = make_float2(v[2], v[3]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) ql_put<BF>(lds, at + e * P, v[e]);
            }
        }
    } else {
        constexpr int C = KCONT ? QL_KC : R, NC = KCONT ? R : QL_KC, PER = NC * C / QL_THREADS;
#pragma unroll
        for (int j = 0; j < 4 * PER; ++j) {
            const int blk = j / PER, idx = tid + (j % PER) * QL_THREADS;
            const int c = idx % C, run = idx / C;
            const int r = KCONT ? run : c, k = KCONT ? c : run;
            float v = 0.f;
            if (r0 + r < op.rmax && k0 + k < kend) v = op.p[blk][KCONT ? (r0 + r) * op.ld + k0 + k : (k0 + k) * op.ld + r0 + r];
            if (SUM) bsum[blk][0] += v;
            ql_put<BF>(lds, (blk * R + r) * P + k, v);
        }
    }
}

// the 16 signed block products of one k step, for the wave's RT row tiles (rows (wr*RT + t)*16 .. of A, wc*16 .. of B)
template <int MODE, bool BF, int RT>
__device__ __forceinline__ void ql_mma(const void* As, const void* Bs, f32x4 (&acc)[RT][4], int wr, int wc, int lr, int lq) {
    constexpr unsigned FLIP = ql_flips(MODE);
    constexpr int TM = 32 * RT;
    if (!BF) {
        const float* A = reinterpret_cast<const float*>(As);
        const float* B = reinterpret_cast<const float*>(Bs);
#pragma unroll
        for (int kk = 0; kk < QL_KC / 4; ++kk) {
            const int k = 4 * kk + lq;
            float bf[4];
#pragma unroll
            for (int y = 0; y < 4; ++y) bf[y] = B[(y * QL_TW + wc * 16 + lr) * QL_PF + k];
#pragma unroll
            for (int t = 0; t < RT; ++t) {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float a = A[(x * TM + (wr * RT + t) * 16 + lr) * QL_PF + k];
                    const float na = __uint_as_float(__float_as_uint(a) ^ 0x80000000u);
#pragma unroll
                    for (int y = 0; y < 4; ++y)
                        acc[t][x ^ y] = __builtin_amdgcn_mfma_f32_16x16x4f32(((FLIP >> (4 * x + y)) & 1u) ? na : a, bf[y], acc[t][x ^ y], 0, 0, 0);
                }
            }
        }
    } else {
        const unsigned short* A = reinterpret_cast<const unsigned short*>(As);
        const unsigned short* B = reinterpret_cast<const unsigned short*>(Bs);
        u32x4 bf[4];
#pragma unroll
        for (int y = 0; y < 4; ++y) bf[y] = *reinterpret_cast<const u32x4*>(B + (y * QL_TW + wc * 16 + lr) * QL_PB + 8 * lq);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const u32x4 a = *reinterpret_cast<const u32x4*>(A + (x * TM + (wr * RT + t) * 16 + lr) * QL_PB + 8 * lq);
                const u32x4 na = a ^ 0x80008000u;
#pragma unroll
                for (int y = 0; y < 4; ++y)
                    acc[t][x ^ y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ((FLIP >> (4 * x + y)) & 1u) ? na : a),
                                                                            __builtin_bit_cast(bf16x8, bf[y]), acc[t][x ^ y], 0, 0, 0);
            }
        }
    }
}

// grid (A row tiles, B row tiles, slices [dcomp; else 1]), block 256
template <int MODE, bool BF, int RT>
__global__ __launch_bounds__(QL_THREADS) void ql_kernel(QlArgs g) {
    constexpr int TM = 32 * RT, ESZ = BF ? 2 : 4, P = BF ? QL_PB : QL_PF;
    static_assert((4 * TM + 4 * QL_TW) * P * ESZ >= QL_THREADS * 16 * 4, "the bias reduction reuses the tiles");
    __shared__ __attribute__((aligned(16))) unsigned char lds[(4 * TM + 4 * QL_TW) * P * ESZ];
    void* As = lds;
    void* Bs = lds + 4 * TM * P * ESZ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4, wr = wave & 1, wc = wave >> 1;
    const long r0 = (long)blockIdx.x * TM, w0 = (long)blockIdx.y * QL_TW;
    long kbeg = 0, kend = g.kw;
    if (MODE == QL_DW) {
        kbeg = (long)blockIdx.z * g.rows;
        kend = kbeg + g.rows < g.kw ? kbeg + g.rows : g.kw;
    }
    const bool sum = MODE == QL_DW && g.pbias != nullptr && blockIdx.x == 0;
    f32x4 acc[RT][4];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[4][4] = {};
    for (long k0 = kbeg; k0 < kend; k0 += QL_KC) {
        ql_stage<MODE != QL_DW, BF, TM, false>(As, g.a, r0, k0, kend, bsum);
        if (MODE == QL_DW && sum) ql_stage<false, BF, QL_TW, true>(Bs, g.b, w0, k0, kend, bsum);
        else ql_stage<MODE == QL_DX, BF, QL_TW, false>(Bs, g.b, w0, k0, kend, bsum);
        __syncthreads();
        ql_mma<MODE, BF, RT>(As, Bs, acc, wr, wc, lr, lq);
        __syncthreads();
    }
    // accumulator element e of lane (lr, lq): A row 4*lq + e, B row lr of the 16 x 16 tile
    const long w = w0 + wc * 16 + lr;
    if (w < g.b.rmax) {
#pragma unroll
        for (int t = 0; t < RT; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long r = r0 + (wr * RT + t) * 16 + 4 * lq + e;
                if (r >= g.a.rmax) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (MODE == QL_DW) {  // workspace[slice][c][i][o]
                        g.out[((long)blockIdx.z * 4 + c) * g.ldo + r * g.outw + w] = acc[t][c][e];
                    } else {
                        const long col = c * g.outw + w;
                        g.out[r * g.ldo + col] = acc[t][c][e] + (g.bias != nullptr ? g.bias[col] : 0.f);
                    }
                }
            }
        }
    }
    if (sum) {  // (block-uniform) column sums of the staged dY: the threads of a column, in ascending order
        float* red = reinterpret_cast<float*>(lds);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[tid * 16 + q * 4 + e] = bsum[q][e];
        __syncthreads();
        if (tid < 4 * QL_TW) {
            const int q = tid >> 5, o = tid & 31;
            float s = 0.f;
            if (g.b.vec) {
                for (int m = 0; m < QL_THREADS / 8; ++m) s += red[(m * 8 + (o >> 2)) * 16 + q * 4 + (o & 3)];
            } else {
                for (int m = 0; m < QL_THREADS / 32; ++m) s += red[(m * 32 + o) * 16 + q * 4];
            }
            if (w0 + o < g.b.rmax) g.pbias[((long)blockIdx.z * 4 + q) * g.outw + w0 + o] = s;
        }
    }
}

// dcomp[c][i][o] = (accumulate ? dcomp : 0) + sum over the slices in ascending order; dbias likewise without the old value
__global__ __launch_bounds__(256) void ql_reduce_kernel(const float* __restrict__ ws, int slices, long IO, long O, int accumulate,
                                                        QlPtrsOut tab, float* __restrict__ base, float* __restrict__ dbias) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < 4 * IO) {
        float s = 0.f;
        for (int sl = 0; sl < slices; ++sl) s += ws[(long)sl * 4 * IO + idx];
        const int c = (int)(idx / IO);
        const long at = idx - c * IO;
        float* dst = base != nullptr ? base + c * IO : tab.p[c];
        if (accumulate) s += dst[at];
        dst[at] = s;
    } else if (dbias != nullptr && idx < 4 * IO + 4 * O) {
        const long j = idx - 4 * IO;
        const float* pb = ws + (long)slices * 4 * IO;
        float s = 0.f;
        for (int sl = 0; sl < slices; ++sl) s += pb[(long)sl * 4 * O + j];
        dbias[j] = s;
    }
}

// ---- the wide family (variant 1): 128 x 64 block pairs streamed through two LDS stages -----------------------------------
// A workgroup (four waves, 2 x 2) owns 128 rows of A by 64 rows of B and all four accumulator sets; a wave owns 4 x 2 MFMA
// tiles of each set, 128 accumulator registers that stay put for the whole reduction.  Per k step (32 in bf16 mode, 16 in
// fp32 mode: two stages of (4*128 + 4*64) rows are 120 KB resp. 108 KB of the CU's 160 KB) the global loads of step k + 1 go
// into registers BEFORE the MFMAs of step k and are rounded and stored to the other stage AFTER them; one barrier per step
// separates the reads of a stage from its next writes.  Pitches, load widths, zero fill, rounding and the sign flip are
// those of the family above; the fp32 pitch of 18 floats spreads 16 rows x 2 k over 32 banks as 34 does.  The matrix
// instruction takes the B fragment first, so that a lane's four accumulator elements run along the row index of B, which
// is contiguous in the output: one 16-byte store per tile and row where pitch and base allow.
constexpr int QW_TM = 128, QW_TW = 64, QW_RT = 4;
// dcomp takes 32 rows of B: its slices are bounded by the workspace, and 128 x 32 block pairs are twice the workgroups
constexpr int qw_tw(int mode) { return mode == QL_DW ? 32 : QW_TW; }
// registers (16 bytes each) a thread holds of one operand's four [R][KC] tiles
constexpr int qw_nv(int R, int KC) { return 4 * ((R * KC / 4 + QL_THREADS - 1) / QL_THREADS); }
template <bool BF>
struct QwGeo {
    static constexpr int KC = BF ? 32 : 16;                                      // k per step
    static constexpr int P = BF ? KC + 8 : KC + 2;                                // LDS row pitch (elements)
    static constexpr int STAGE = 4 * (QW_TM + QW_TW) * P * (BF ? 2 : 4);          // bytes of one stage
};
static_assert(2 * QwGeo<true>::STAGE <= 160 * 1024 && 2 * QwGeo<false>::STAGE <= 160 * 1024, "both stages fit the LDS of a gfx950 CU");
static_assert(QwGeo<true>::STAGE >= QL_THREADS * 16 * 4 && QwGeo<false>::STAGE >= QL_THREADS * 16 * 4, "the bias reduction reuses a stage");

// The thread's share of the four [R][KC] tiles of one operand, global memory -> registers (element order of ql_stage).
// R * KC / 256 16-byte loads, or four times as many 4-byte loads into the same registers.  No load is predicated: an index
// past the valid part of the tile (rlim rows, klim of k, both >= 1) is clamped into it, and qw_store writes zero in its
// place - held from here, the predicates of up to 96 loads in flight cost more scalar registers than there are.  The
// address is a uniform 64-bit corner and a 32-bit offset (at most 127 * 2^22 + 2^20 elements).
template <bool KCONT, int R, int KC>
__device__ __forceinline__ void qw_load(f32x4 (&v)[qw_nv(R, KC)], const QlOp& op, long r0, long k0, int rlim, int klim) {
    const int tid = threadIdx.x;
    const long corner = KCONT ? r0 * op.ld + k0 : k0 * op.ld + r0;
    const unsigned ld = (unsigned)op.ld;
    if (op.vec) {  // (the contiguous extent is a multiple of 4: all four or none)
        // (32 x 16 fp32: half a pass per block, the upper threads store nothing)
        constexpr int C4 = (KCONT ? KC : R) / 4, NC = KCONT ? R : KC, PER = (NC * C4 + QL_THREADS - 1) / QL_THREADS;
#pragma unroll
        for (int j = 0; j < 4 * PER; ++j) {
            const int blk = j / PER, idx = tid + (j % PER) * QL_THREADS;
            const int c4 = idx % C4, run = idx / C4;
            const int r = KCONT ? run : 4 * c4, k = KCONT ? 4 * c4 : run;
            const int rc = min(r, rlim - (KCONT ? 1 : 4)), kc = min(k, klim - (KCONT ? 4 : 1));
            v[j] = *reinterpret_cast<const f32x4*>(op.p[blk] + corner + (KCONT ? rc * ld + kc : kc * ld + rc));
        }
    } else {
        constexpr int C = KCONT ? KC : R, NC = KCONT ? R : KC, PER = NC * C / QL_THREADS;
#pragma unroll
        for (int j = 0; j < 4 * PER; ++j) {
            const int blk = j / PER, idx = tid + (j % PER) * QL_THREADS;
            const int c = idx % C, run = idx / C;
            const int r = KCONT ? run : c, k = KCONT ? c : run;
            const int rc = min(r, rlim - 1), kc = min(k, klim - 1);
            v[j / 4][j % 4] = (op.p[blk] + corner)[KCONT ? rc * ld + kc : kc * ld + rc];
        }
    }
}

// all ones where r < rlim and k < klim, else zero, in vector arithmetic: as compares, the masks of a stage's values would
// be held in scalar register pairs
__device__ __forceinline__ unsigned qw_inside(int r, int k, int rlim, int klim) { return (unsigned)(((r - rlim) & (k - klim)) >> 31); }

// ... and registers -> one LDS stage as [block][row][k], zero outside rlim / klim, rounded to bf16 in bf16 mode.  SUM (dcomp's dY): the thread also
// adds what it holds into bsum[blk][e]; its column(s) are the same in every step (256 % (R / 4) == 256 % R == 0).
template <bool KCONT, bool BF, int R, int KC, bool SUM>
__device__ __forceinline__ void qw_store(void* lds, const f32x4 (&v)[qw_nv(R, KC)], int vec, int rlim, int klim, float (&bsum)[4][4]) {
    constexpr int P = QwGeo<BF>::P;
    const int tid = threadIdx.x;
    if (vec) {
        constexpr int C4 = (KCONT ? KC : R) / 4, NC = KCONT ? R : KC, PER = (NC * C4 + QL_THREADS - 1) / QL_THREADS;
#pragma unroll
        for (int j = 0; j < 4 * PER; ++j) {
            const int blk = j / PER, idx = tid + (j % PER) * QL_THREADS;
            const int c4 = idx % C4, run = idx / C4;
            const int r = KCONT ? run : 4 * c4, k = KCONT ? 4 * c4 : run;
            if (NC * C4 % QL_THREADS != 0 && idx >= NC * C4) continue;
            const f32x4 x = __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, v[j]) & qw_inside(r, k, rlim, klim));
            if (SUM) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bsum[blk][e] += x[e];
            }
            const int at = (blk * R + r) * P + k;
            if (KCONT) {
                if (BF) {
                    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(lds) + at) = make_uint2(pk_pack_bf2(x[0], x[1]), pk_pack_bf2(x[2], x[3]));
                } else {
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(lds) + at) = make_float2(x[0], x[1]);
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(lds) + at + 2) = make_float2(x[2], x[3]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) ql_put<BF>(lds, at + e * P, x[e]);
            }
        }
    } else {
        constexpr int C = KCONT ? KC : R, NC = KCONT ? R : KC, PER = NC * C / QL_THREADS;
#pragma unroll
        for (int j = 0; j < 4 * PER; ++j) {
            const int blk = j / PER, idx = tid + (j % PER) * QL_THREADS;
            const int c = idx % C, run = idx / C;
            const int r = KCONT ? run : c, k = KCONT ? c : run;
            const float x = __uint_as_float(__float_as_uint(v[j / 4][j % 4]) & qw_inside(r, k, rlim, klim));
            if (SUM) bsum[blk][0] += x;
            ql_put<BF>(lds, (blk * R + r) * P + k, x);
        }
    }
}

// the 16 signed block products of one k step for the wave's 4 x CT tiles (rows (4*wr + t)*16 .. of A, (CT*wc + u)*16 .. of B):
// 4 * CT B fragments stay in registers, each of the 16 A fragments is read once, flipped once and feeds 4 * CT matrix
// instructions
template <int MODE, bool BF>
__device__ __forceinline__ void qw_mma(const void* As, const void* Bs, f32x4 (&acc)[QW_RT][qw_tw(MODE) / 32][4], int wr, int wc, int lr, int lq) {
    constexpr unsigned FLIP = ql_flips(MODE);
    constexpr int BT = qw_tw(MODE), BCT = BT / 32;  // rows of B per workgroup, MFMA tiles of them per wave
    constexpr int KC = QwGeo<BF>::KC, P = QwGeo<BF>::P;
    if (!BF) {
        const float* A = reinterpret_cast<const float*>(As);
        const float* B = reinterpret_cast<const float*>(Bs);
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const int k = 4 * kk + lq;
            float bf[BCT][4];
#pragma unroll
            for (int u = 0; u < BCT; ++u)
#pragma unroll
                for (int y = 0; y < 4; ++y) bf[u][y] = B[(y * BT + (wc * BCT + u) * 16 + lr) * P + k];
#pragma unroll
            for (int t = 0; t < QW_RT; ++t) {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float a = A[(x * QW_TM + (wr * QW_RT + t) * 16 + lr) * P + k];
                    const float na = __uint_as_float(__float_as_uint(a) ^ 0x80000000u);
#pragma unroll
                    for (int u = 0; u < BCT; ++u)
#pragma unroll
                        for (int y = 0; y < 4; ++y)
                            acc[t][u][x ^ y] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[u][y], ((FLIP >> (4 * x + y)) & 1u) ? na : a, acc[t][u][x ^ y], 0, 0, 0);
                }
            }
        }
    } else {
        const unsigned short* A = reinterpret_cast<const unsigned short*>(As);
        const unsigned short* B = reinterpret_cast<const unsigned short*>(Bs);
        u32x4 bf[BCT][4];
#pragma unroll
        for (int u = 0; u < BCT; ++u)
#pragma unroll
            for (int y = 0; y < 4; ++y) bf[u][y] = *reinterpret_cast<const u32x4*>(B + (y * BT + (wc * BCT + u) * 16 + lr) * P + 8 * lq);
        // the A fragments of row tile t + 1 are read under the 32 MFMAs of row tile t; the scheduling fence keeps the
        // compiler from hoisting all 16 reads (and their flipped copies) to the top, which would not fit the registers
        u32x4 a[2][4];
#pragma unroll
        for (int x = 0; x < 4; ++x) a[0][x] = *reinterpret_cast<const u32x4*>(A + (x * QW_TM + wr * QW_RT * 16 + lr) * P + 8 * lq);
#pragma unroll
        for (int t = 0; t < QW_RT; ++t) {
            if (t + 1 < QW_RT) {
#pragma unroll
                for (int x = 0; x < 4; ++x)
                    a[(t + 1) & 1][x] = *reinterpret_cast<const u32x4*>(A + (x * QW_TM + (wr * QW_RT + t + 1) * 16 + lr) * P + 8 * lq);
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const u32x4 na = a[t & 1][x] ^ 0x80008000u;
#pragma unroll
                for (int u = 0; u < BCT; ++u)
#pragma unroll
                    for (int y = 0; y < 4; ++y)
                        acc[t][u][x ^ y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bf[u][y]),
                                                                                   __builtin_bit_cast(bf16x8, ((FLIP >> (4 * x + y)) & 1u) ? na : a[t & 1][x]),
                                                                                   acc[t][u][x ^ y], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// grid (B row tiles * A row tiles with the B tiles running fastest - the workgroups that share 128 rows of A are
// neighbours in time -, 1, slices [dcomp; else 1]), block 256, 2 * STAGE bytes of dynamic LDS
template <int MODE, bool BF>
__global__ __launch_bounds__(QL_THREADS) void ql_wide_kernel(QlArgs g, int wtiles, int outvec) {
    constexpr int KC = QwGeo<BF>::KC, STAGE = QwGeo<BF>::STAGE, ABYTES = 4 * QW_TM * QwGeo<BF>::P * (BF ? 2 : 4);
    constexpr bool AK = MODE != QL_DW, BK = MODE == QL_DX;  // k is the contiguous index of A / of B
    constexpr int BT = qw_tw(MODE), BCT = BT / 32;  // rows of B per workgroup, MFMA tiles of them per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char qw_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4, wr = wave & 1, wc = wave >> 1;
    const long r0 = (long)(blockIdx.x / wtiles) * QW_TM, w0 = (long)(blockIdx.x % wtiles) * BT;
    long kbeg = 0, kend = g.kw;
    if (MODE == QL_DW) {
        kbeg = (long)blockIdx.z * g.rows;
        kend = kbeg + g.rows < g.kw ? kbeg + g.rows : g.kw;
    }
    const bool sum = MODE == QL_DW && g.pbias != nullptr && r0 == 0;
    f32x4 acc[QW_RT][BCT][4];
#pragma unroll
    for (int t = 0; t < QW_RT; ++t)
#pragma unroll
        for (int u = 0; u < BCT; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][u][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[4][4] = {};
    f32x4 ra[qw_nv(QW_TM, KC)], rb[qw_nv(BT, KC)];
    // the valid part of the tiles: rows of A, rows of B (fixed) and k of the step in flight, all >= 1
    const int alim = (int)(g.a.rmax - r0 < QW_TM ? g.a.rmax - r0 : QW_TM), blim = (int)(g.b.rmax - w0 < BT ? g.b.rmax - w0 : BT);
    int klim = (int)(kend - kbeg < KC ? kend - kbeg : KC);
    qw_load<AK, QW_TM, KC>(ra, g.a, r0, kbeg, alim, klim);
    qw_load<BK, BT, KC>(rb, g.b, w0, kbeg, blim, klim);
    qw_store<AK, BF, QW_TM, KC, false>(qw_lds, ra, g.a.vec, alim, klim, bsum);
    if (MODE == QL_DW && sum) qw_store<BK, BF, BT, KC, true>(qw_lds + ABYTES, rb, g.b.vec, blim, klim, bsum);
    else qw_store<BK, BF, BT, KC, false>(qw_lds + ABYTES, rb, g.b.vec, blim, klim, bsum);
    __syncthreads();
    int cur = 0;
    for (long k0 = kbeg; k0 < kend; k0 += KC) {  // (trip count: the slice's rows / KC, known at launch)
        const bool more = k0 + KC < kend;
        if (more) {
            klim = (int)(kend - k0 - KC < KC ? kend - k0 - KC : KC);
            qw_load<AK, QW_TM, KC>(ra, g.a, r0, k0 + KC, alim, klim);
            qw_load<BK, BT, KC>(rb, g.b, w0, k0 + KC, blim, klim);
        }
        qw_mma<MODE, BF>(qw_lds + cur * STAGE, qw_lds + cur * STAGE + ABYTES, acc, wr, wc, lr, lq);
        if (more) {
            unsigned char* nxt = qw_lds + (cur ^ 1) * STAGE;
            qw_store<AK, BF, QW_TM, KC, false>(nxt, ra, g.a.vec, alim, klim, bsum);
            if (MODE == QL_DW && sum) qw_store<BK, BF, BT, KC, true>(nxt + ABYTES, rb, g.b.vec, blim, klim, bsum);
            else qw_store<BK, BF, BT, KC, false>(nxt + ABYTES, rb, g.b.vec, blim, klim, bsum);
        }
        __syncthreads();  // stage cur is read, stage cur ^ 1 is written
        cur ^= 1;
    }
    // accumulator element e of lane (lr, lq): B row 4*lq + e, A row lr of the 16 x 16 tile
#pragma unroll
    for (int t = 0; t < QW_RT; ++t) {
        const long r = r0 + (wr * QW_RT + t) * 16 + lr;
        if (r >= g.a.rmax) continue;
#pragma unroll
        for (int u = 0; u < BCT; ++u) {
            const long w = w0 + (wc * BCT + u) * 16 + 4 * lq;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // dcomp: workspace[slice][c][i][o];  forward / dX: block c of row r
                float* dst = MODE == QL_DW ? g.out + ((long)blockIdx.z * 4 + c) * g.ldo + r * g.outw + w : g.out + r * g.ldo + c * g.outw + w;
                f32x4 o = acc[t][u][c];
                if (MODE != QL_DW && g.bias != nullptr) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (w + e < g.b.rmax) o[e] += g.bias[c * g.outw + w + e];
                }
                if (outvec) {  // (the width is a multiple of 4: all four or none)
                    if (w < g.b.rmax) *reinterpret_cast<f32x4*>(dst) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (w + e < g.b.rmax) dst[e] = o[e];
                }
            }
        }
    }
    if (sum) {  // (block-uniform) column sums of the staged dY: the threads of a column, in ascending order
        float* red = reinterpret_cast<float*>(qw_lds);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[tid * 16 + q * 4 + e] = bsum[q][e];
        __syncthreads();
        const int q = tid / BT, o = tid % BT;
        float s = 0.f;
        if (g.b.vec) {
            for (int m = 0; m < QL_THREADS / (BT / 4); ++m) s += red[(m * (BT / 4) + (o >> 2)) * 16 + q * 4 + (o & 3)];
        } else {
            for (int m = 0; m < QL_THREADS / BT; ++m) s += red[(m * BT + o) * 16 + q * 4];
        }
        if (tid < 4 * BT && w0 + o < g.b.rmax) g.pbias[((long)blockIdx.z * 4 + q) * g.outw + w0 + o] = s;
    }
}

template <int MODE>
int qw_launch(hipStream_t s, bool bf, dim3 grid, const QlArgs& g, int wtiles) {
    const int outvec = g.outw % 4 == 0 && g.ldo % 4 == 0 && ((uintptr_t)g.out & 15) == 0;
    const void* k = bf ? (const void*)ql_wide_kernel<MODE, true> : (const void*)ql_wide_kernel<MODE, false>;
    const size_t lds = 2 * (bf ? QwGeo<true>::STAGE : QwGeo<false>::STAGE);
    if (int rc = pk_grant_dynamic_lds(k, lds)) return rc;
    if (bf) hipLaunchKernelGGL((ql_wide_kernel<MODE, true>), grid, dim3(QL_THREADS), lds, s, g, wtiles, outvec);
    else hipLaunchKernelGGL((ql_wide_kernel<MODE, false>), grid, dim3(QL_THREADS), lds, s, g, wtiles, outvec);
    PK_LAUNCH_CHECK();
    return 0;
}

// Which family serves a call: -1 the rule, 0 / 1 forced (pk_quat_linear_set_variant).  The rule counts the 128 x 64 block
// pairs of the pass's output (for dcomp: of the rows it reduces over) and takes the wide family from the smallest measured
// row count on at which it beat the other by more than the 3 % spread between boxes, forward and forward + backward, fp32
// and bf16 (profiles/quat_linear.json, 1024 -> 1024 on 256 CUs): 16 000 rows = 500 pairs, about two per CU.  At 2 048 rows
// (64 pairs) it loses or ties.  The count scales with the CUs of the device.
int g_ql_variant = -1;
constexpr long QW_PAIRS = 500, QW_PAIRS_CUS = 256;
int ql_variant(int pass, int prec, int64_t N, int I, int O) {
    if (g_ql_variant >= 0) return g_ql_variant;
    // only 1024 -> 1024 is measured: a call whose components do not fill one wide tile (the B rows of the pass, for dcomp
    // also its 128 A rows) would run mostly padding there and stays where it was
    if (pass == QL_DW ? (I < QW_TM || O < qw_tw(QL_DW)) : (pass == QL_DX ? I : O) < QW_TW) return 0;
    const long pairs = (long)((N + QW_TM - 1) / QW_TM) * (((pass == QL_DX ? I : O) + QW_TW - 1) / QW_TW);
    (void)prec;  // (one threshold serves both precisions today)
    return pairs * QW_PAIRS_CUS >= QW_PAIRS * pk_num_cu() ? 1 : 0;
}

bool ql_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// slices of the rows and rows per slice (a multiple of the k step): a function of the shape alone
int ql_slices(int64_t N, int I, int O, long* rows) {
    const long tiles = (long)((I + 31) / 32) * ((O + QL_TW - 1) / QL_TW);
    long s = (QL_FILL + tiles - 1) / tiles;
    const long most = (N + QL_MIN_SLICE - 1) / QL_MIN_SLICE;
    if (s > most) s = most;
    if (s > QL_MAX_SLICES) s = QL_MAX_SLICES;
    if (s < 1) s = 1;
    const long per = ((N + s - 1) / s + QL_KC - 1) / QL_KC * QL_KC;
    *rows = per;
    return (int)((N + per - 1) / per);
}

int ql_check(const char* who, int prec, int64_t N, int I, int O, const void* table, const void* base) {
    PK_REQUIRE(prec == PK_PREC_F32 || prec == PK_PREC_BF16, "%s: prec = %d (PK_PREC_F32 or PK_PREC_BF16)", who, prec);
    PK_REQUIRE(N >= 1 && I >= 1 && O >= 1, "%s: N = %lld rows of components [%d, %d] must be positive", who, (long long)N, I, O);
    PK_REQUIRE(I <= (1 << 20) && O <= (1 << 20) && (long)I * O <= (1L << 30) && N <= (1LL << 31) - 4096 &&
                   N <= (1LL << 40) / (4LL * (I > O ? I : O)),
               "%s: N = %lld rows of components [%d, %d] are out of range (I, O <= 2^20, I * O <= 2^30, N < 2^31, N * 4 * max(I, O) <= 2^40)",
               who, (long long)N, I, O);
    PK_REQUIRE((table != nullptr) != (base != nullptr), "%s: exactly one of the pointer table and the base pointer must be given", who);
    return 0;
}

// the four components as one operand; *cvec: they may be read with 16-byte loads
int ql_comps(const char* who, const float* const* comps, const float* base, int I, int O, QlOp* op) {
    bool al = O % 4 == 0;
    for (int c = 0; c < 4; ++c) {
        const float* p = base != nullptr ? base + (long)c * I * O : comps[c];
        PK_REQUIRE(p != nullptr, "%s: component %d of the pointer table is NULL", who, c);
        op->p[c] = p;
        al = al && ql_aligned(p);
    }
    op->ld = O;
    op->vec = al;
    return 0;
}

void ql_blocks(QlOp* op, const float* m, int width, long rmax) {
    for (int b = 0; b < 4; ++b) op->p[b] = m + (long)b * width;
    op->ld = 4L * width;
    op->rmax = rmax;
    op->vec = width % 4 == 0 && ql_aligned(m);
}

// forward (dx = 0) and dX (dx = 1): in [N][4*KW], out [N][4*OW]
int ql_rows(void* stream, int dx, int prec, int64_t N, int KW, int OW, const float* in, const QlOp& comps, const float* bias, float* out) {
    QlArgs g = {};
    ql_blocks(&g.a, in, KW, N);
    g.b = comps;
    g.b.rmax = OW;
    g.kw = KW;
    g.out = out, g.ldo = 4L * OW, g.outw = OW, g.bias = bias;
    if (ql_variant(dx ? QL_DX : QL_FWD, prec, N, dx ? OW : KW, dx ? KW : OW)) {
        const long wtw = (OW + QW_TW - 1) / QW_TW;
        const dim3 wgrid((unsigned)((N + QW_TM - 1) / QW_TM * wtw));
        return dx ? qw_launch<QL_DX>(pk_stream(stream), prec == PK_PREC_BF16, wgrid, g, (int)wtw)
                  : qw_launch<QL_FWD>(pk_stream(stream), prec == PK_PREC_BF16, wgrid, g, (int)wtw);
    }
    const long wt = (OW + QL_TW - 1) / QL_TW;
    const int rt = (N + 63) / 64 * wt >= QL_FILL_RT2 ? 2 : 1;
    const dim3 grid((unsigned)((N + 32 * rt - 1) / (32 * rt)), (unsigned)wt), block(QL_THREADS);
    hipStream_t s = pk_stream(stream);
    const bool bf = prec == PK_PREC_BF16;
#define QL_LAUNCH(MODE)                                                                   \
    do {                                                                                  \
        if (bf && rt == 2) hipLaunchKernelGGL((ql_kernel<MODE, true, 2>), grid, block, 0, s, g);   \
        else if (bf) hipLaunchKernelGGL((ql_kernel<MODE, true, 1>), grid, block, 0, s, g);          \
        else if (rt == 2) hipLaunchKernelGGL((ql_kernel<MODE, false, 2>), grid, block, 0, s, g);    \
        else hipLaunchKernelGGL((ql_kernel<MODE, false, 1>), grid, block, 0, s, g);                 \
    } while (0)
    if (dx) QL_LAUNCH(QL_DX);
    else QL_LAUNCH(QL_FWD);
#undef QL_LAUNCH
    PK_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// the argument limits of pk_quat_linear_work_floats
static bool ql_in_range(int64_t N, int I, int O) {
    return !(N < 1 || I < 1 || O < 1 || I > (1 << 20) || O > (1 << 20) || (long)I * O > (1L << 30) || N > (1LL << 31) - 4096);
}

extern "C" int64_t pk_quat_linear_work_floats(int64_t N, int I, int O) {
    if (!ql_in_range(N, I, O)) return 0;
    long rows;
    const int64_t s = ql_slices(N, I, O, &rows);
    return s * (4LL * I * O + 4LL * O);
}

extern "C" void pk_quat_linear_set_variant(int v) { g_ql_variant = (v == 0 || v == 1) ? v : -1; }

extern "C" int pk_quat_linear_variant(int pass, int prec, int64_t N, int I, int O) {
    if (pass < QL_FWD || pass > QL_DW || (prec != PK_PREC_F32 && prec != PK_PREC_BF16) || !ql_in_range(N, I, O)) return 0;
    return ql_variant(pass, prec, N, I, O);
}

extern "C" int pk_quat_linear_fwd(void* stream, int prec, int64_t N, int I, int O, const float* X, const float* const* comps,
                                  const float* base, const float* bias, float* Y) {
    if (int rc = ql_check("pk_quat_linear_fwd", prec, N, I, O, comps, base)) return rc;
    PK_REQUIRE(X != nullptr && Y != nullptr, "pk_quat_linear_fwd: X or Y are NULL");
    QlOp c = {};
    if (int rc = ql_comps("pk_quat_linear_fwd", comps, base, I, O, &c)) return rc;
    return ql_rows(stream, 0, prec, N, I, O, X, c, bias, Y);
}

extern "C" int pk_quat_linear_bwd_x(void* stream, int prec, int64_t N, int I, int O, const float* dY, const float* const* comps,
                                    const float* base, float* dX) {
    if (int rc = ql_check("pk_quat_linear_bwd_x", prec, N, I, O, comps, base)) return rc;
    PK_REQUIRE(dY != nullptr && dX != nullptr, "pk_quat_linear_bwd_x: dY or dX are NULL");
    QlOp c = {};
    if (int rc = ql_comps("pk_quat_linear_bwd_x", comps, base, I, O, &c)) return rc;
    return ql_rows(stream, 1, prec, N, O, I, dY, c, nullptr, dX);
}

extern "C" int pk_quat_linear_bwd_w(void* stream, int prec, int64_t N, int I, int O, const float* X, const float* dY, float beta,
                                    float* const* dcomps, float* dbase, float* dbias, float* workspace) {
    if (int rc = ql_check("pk_quat_linear_bwd_w", prec, N, I, O, dcomps, dbase)) return rc;
    PK_REQUIRE(X != nullptr && dY != nullptr && workspace != nullptr, "pk_quat_linear_bwd_w: X, dY or the workspace are NULL");
    PK_REQUIRE(beta == 0.0f || beta == 1.0f, "pk_quat_linear_bwd_w: beta = %g (0 overwrites, 1 accumulates)", (double)beta);
    QlPtrsOut tab = {};
    if (dcomps != nullptr) {
        for (int c = 0; c < 4; ++c) {
            PK_REQUIRE(dcomps[c] != nullptr, "pk_quat_linear_bwd_w: component %d of the pointer table is NULL", c);
            tab.p[c] = dcomps[c];
        }
    }
    long rows;
    const int slices = ql_slices(N, I, O, &rows);
    const long IO = (long)I * O;
    QlArgs g = {};
    ql_blocks(&g.a, X, I, I);
    ql_blocks(&g.b, dY, O, O);
    g.kw = N, g.rows = rows;
    g.out = workspace, g.ldo = IO, g.outw = O;
    g.pbias = dbias != nullptr ? workspace + (long)slices * 4 * IO : nullptr;
    const dim3 grid((unsigned)((I + 31) / 32), (unsigned)((O + QL_TW - 1) / QL_TW), (unsigned)slices), block(QL_THREADS);
    hipStream_t s = pk_stream(stream);
    if (ql_variant(QL_DW, prec, N, I, O)) {  // the same slices (every one of them holds rows), a quarter .. an eighth of the workgroups
        const long wtw = (O + qw_tw(QL_DW) - 1) / qw_tw(QL_DW);
        const dim3 wgrid((unsigned)((I + QW_TM - 1) / QW_TM * wtw), 1, (unsigned)slices);
        if (int rc = qw_launch<QL_DW>(s, prec == PK_PREC_BF16, wgrid, g, (int)wtw)) return rc;
    } else {
        if (prec == PK_PREC_BF16) hipLaunchKernelGGL((ql_kernel<QL_DW, true, 1>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((ql_kernel<QL_DW, false, 1>), grid, block, 0, s, g);
        PK_LAUNCH_CHECK();
    }
    const long total = 4 * IO + (dbias != nullptr ? 4L * O : 0);
    hipLaunchKernelGGL(ql_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, workspace, slices, IO, (long)O,
                       beta != 0.0f ? 1 : 0, tab, dbase, dbias);
    PK_LAUNCH_CHECK();
    return 0;
}
