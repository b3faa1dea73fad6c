// pk_rec_persist2_dirs.hip - perf-mode persistent time loops of a TORCH-LAYOUT bidirectional layer (LSTM_cudnn /
// RNN_cudnn: torch.nn.LSTM / nn.RNN keep one weight set per direction): BOTH directions in ONE launch, forward and BPTT.
//
// The engine's own bidirectional layers share one recurrent matrix between the directions, so pk_rec_persist2.hip holds
// one U per launch and a torch-layout layer used to take two launches, each half empty (a step costs the same for 8
// rows as for 16).  Here a launch carries two weight sets:
//
//   * clusters are DIRECTION-PURE.  A wave keeps its 16 units' slice of ONE U in registers for all T steps - two do
//     not fit - so direction d gets its own ceil(B / rpc) clusters: cluster c of the grid's C = 2 * Cd serves direction
//     c / Cd, rows b = (c % Cd) * rpc ... of it, even where 2B <= 16 rows would fit one MFMA tile.  Everything that
//     depends on the direction - the U / P / pscale / pshift slab, the time order, the column half of Y / Yb, the slab
//     of S / dGb / dP2 - is therefore uniform over a workgroup: scalar registers and scalar branches, where the shared-U
//     kernels carry it per lane (per polled chunk, per vector row, per publish piece).
//   * P is [2][T*B][G*H] (slab d = x . W_d^T, indexed by ORIGINAL time: direction 1 reads row (T-1-t)*B + b), pscale /
//     pshift are [2][G*H], U is [2][G*H][H].  Y, S, Yb, dP2, dGb keep the layouts of pk_rec_fwd_bf16 / pk_rec_bwd_bf16
//     with bidir = 1: the reversed half is stored at its original time index in columns H:2H, so the caller needs no
//     time-reversed copy of its input and no join of two outputs.
//   * per-row arithmetic is that of the kernels pk_rec_{fwd,bwd}_bf16 launch by default for the cell, so every row comes
//     out bit-identical to the single-direction launch of its direction:
//       RNN   four waves per workgroup, one accumulator per gate over k = 0..17 (forward); two accumulators over even /
//             odd k-steps (backward) - pk_rec_persist2.hip / pk_rec_persist3.hip;
//       LSTM  eight waves, two per group of 16 units: gate split (f, i) / (o, g) in the forward pass, K split with a
//             partial-sum hand-over in the backward pass - pk_rec_persist2_lstm.hip has the reasoning.
//     One kernel template per pass covers both: PAIR (= LSTM) selects the two-wave form.
//   * the exchange is pk_rec_persist2.hip's: bf16 through L2, 16 bytes at a time, the data is the flag, self-filling
//     PK_R2_FILL_AHEAD steps ahead, XCD-local fast path after the placement handshake, every spin bounded by spin_limit
//     and reported in the host-visible error word.
//
// No recurrent mask (mask_scalar only), no per-step LayerNorm.  Reference: neural_networks.py:153-203, :256-297.
#include <stdlib.h>

#include "pk_rec2_common.h"

namespace {

// what a workgroup's cluster serves
struct DirCluster {
    int dir, b0, nrows;
};
__device__ __forceinline__ DirCluster dir_cluster(const R2Args& a, int c) {
    const int Cd = a.C >> 1;
    const int dir = c >= Cd ? 1 : 0, cl = c - dir * Cd;
    int nrows = a.B - cl * a.rpc;
    nrows = nrows < a.rpc ? nrows : a.rpc;
    return DirCluster{__builtin_amdgcn_readfirstlane(dir), __builtin_amdgcn_readfirstlane(cl * a.rpc),
                      __builtin_amdgcn_readfirstlane(nrows)};
}

// ============================================================================
// forward
// ============================================================================
template <int CELL, int ACT>
__global__ __launch_bounds__(CELL == PK_CELL_LSTM ? 512 : 256, 1) void rec2d_fwd_kernel(R2Args a) {
    const int act = ACT >= 0 ? ACT : a.act;
    constexpr bool PAIR = CELL == PK_CELL_LSTM;
    constexpr int G = pk_cell_gates(CELL), NS = pk_cell_saved(CELL);
    constexpr int NWV = PAIR ? 8 : 4, NT = NWV * 64;
    constexpr int GW = PAIR ? 2 : G;      // gates a wave multiplies
    constexpr int NSW = PAIR ? 3 : NS;    // S slots a wave stages (PAIR: f, i, c / o, g)
    constexpr int LDA = pk_r2_lda_bf16(KPAD);
    constexpr int ATILE = RMAX * LDA * 2;
    constexpr int NCH = (RMAX * (KPAD / 8) + NT - 1) / NT;
    constexpr int WAVE_LDS = (GW + 1 + NSW) * 1024 + 512;  // P stage | Y | S slots | bf16 publish patch
    constexpr int XCH = 2 * ATILE + NWV * WAVE_LDS;        // PAIR hand-over: [4 pairs][2 gates][64 lanes] x 16 bytes
    constexpr int LDS_TRASH = XCH + (PAIR ? 4 * GW * 1024 : 0);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, uw = wave & 3;
    const int half = PAIR ? __builtin_amdgcn_readfirstlane(wave >> 2) : 0;  // PAIR: 0 = gates f, i (+ state, publish); 1 = o, g
    const int g0 = half * GW;
    const int c = blockIdx.x % a.C, p = blockIdx.x / a.C;
    const int H = a.H, Hp = a.Hp, B = a.B, T = a.T, GH = G * H;
    const DirCluster dc = dir_cluster(a, c);
    const int dir = dc.dir, nrows = dc.nrows;
    if (nrows <= 0) return;  // whole workgroup (uniform)
    const int ubase = p * 64 + uw * 16;
    const int unit = ubase + (lane & 15);
    const bool unit_ok = unit < H;
    const int kq = lane >> 4;
    // this direction's slabs
    const float* const Ud = a.U + (size_t)dir * G * H * H;
    const float* const Pd = a.P + (size_t)dir * T * B * GH;
    const float* const pscd = a.pscale + dir * GH;
    const float* const pshd = a.pshift + dir * GH;

    // ---- recurrent weights of my 16 units, my gates -> registers (once): B[k][n] = U_g[unit n][k]
    bf16x8 Bf[GW][KSTEPS];
    {
        const unsigned szU = (unsigned)((size_t)G * H * H * 4);
        const __amdgpu_buffer_rsrc_t rsU = make_rsrc(Ud, szU);
        constexpr int KB = 6;  // six k-steps at a time, fenced: the raw loads must not all be live at once
#pragma unroll
        for (int gg = 0; gg < GW; ++gg) {
            const int g = g0 + gg;
#pragma unroll
            for (int kb = 0; kb < KSTEPS; kb += KB) {
                u32x4 raw[KB][2];
#pragma unroll
                for (int kj = 0; kj < KB; ++kj) {
                    const int k0 = (kb + kj) * 32 + kq * 8;
                    const unsigned off = (unsigned)(((g * H + unit) * H + k0) * 4);
                    raw[kj][0] = __builtin_amdgcn_raw_buffer_load_b128(rsU, (unit_ok && k0 < H) ? off : szU, 0, 0);
                    raw[kj][1] = __builtin_amdgcn_raw_buffer_load_b128(rsU, (unit_ok && k0 + 4 < H) ? off + 16 : szU, 0, 0);
                }
#pragma unroll
                for (int kj = 0; kj < KB; ++kj) {
                    bf16x8 f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int k = (kb + kj) * 32 + kq * 8 + e;
                        const float w = (k < H) ? __uint_as_float(raw[kj][e >> 2][e & 3]) : 0.f;  // beyond H: the next row's data
                        f[e] = (short)pk_f2bf(w);
                    }
                    Bf[gg][kb + kj] = f;
                }
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    float psc[GW], psh[GW];
#pragma unroll
    for (int gg = 0; gg < GW; ++gg) {
        psc[gg] = unit_ok ? pscd[(g0 + gg) * H + unit] : 0.f;
        psh[gg] = unit_ok ? pshd[(g0 + gg) * H + unit] : 0.f;
    }
    for (int i = tid; i < (LDS_TRASH + 16) / 4; i += NT) reinterpret_cast<unsigned*>(smem)[i] = 0u;

    // ---- poll descriptors: chunk ci = (row, col) of the cluster's [nrows][Hp/8] block of h_{t-1}.  Step t reads storage
    // time (dir ? T-t : t-1): one base per chunk, ONE step for the whole workgroup
    const int CPR = Hp >> 3;
    const unsigned TS = (unsigned)B * a.Ypitch * 2u;  // bytes per time slab of Yb
    const unsigned szYb = (unsigned)T * TS;
    const unsigned tstep = dir ? 0u - TS : TS;
    const unsigned t0off = dir ? (unsigned)(T - 1) * TS : 0u;  // byte offset of step 0's slab
    unsigned cbase[NCH];
    int clds[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ci = tid + NT * i;
        const bool ok = ci < nrows * CPR;
        const int row = ok ? ci / CPR : 0, col = ok ? ci - row * CPR : 0;
        cbase[i] = ok ? ((unsigned)(dc.b0 + row) * a.Ypitch + dir * Hp + col * 8) * 2u + t0off : szYb;
        clds[i] = ok ? row * (LDA * 2) + col * 16 : LDS_TRASH;
    }
    // ---- gate-math (C/D) layout: rows kq*4 + r, unit lane&15
    const float msk = a.mask_scalar;
    float rvf[4], hprev[4], cprev[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        rvf[r] = (kq * 4 + r < nrows && unit_ok) ? 1.f : 0.f;
        hprev[r] = 0.f;
        cprev[r] = 0.f;
    }
    // ---- vector layout: row lane>>2, units ubase + (lane&3)*4 .. +3
    const int vrow = lane >> 2, vu0 = ubase + (lane & 3) * 4;
    const int vb = dc.b0 + (vrow < nrows ? vrow : 0);
    int vnv = H - vu0;
    vnv = vnv > 4 ? 4 : (vnv < 0 ? 0 : vnv);
    // wave-uniform: 0 = my 16 units do not straddle H, 1 = they do and H is even, 2 = H is odd
    const int edge = __any(vnv > 0 && vnv < 4) != 0 ? ((H & 1) ? 2 : 1) : 0;
    vnv = vrow < nrows ? vnv : 0;
    // element offsets of my 4 units at storage time 0 / per unit of storage time, for P, Y and S
    const unsigned vP0 = ((unsigned)vb * GH + vu0), vPs = (unsigned)B * GH;
    const unsigned vY0 = ((unsigned)vb * a.YH + dir * H + vu0), vYs = (unsigned)B * a.YH;
    const unsigned vS0 = (((unsigned)dir * T * B + vb) * (NS * H) + vu0), vSs = (unsigned)B * NS * H;
    // ---- publish descriptors (PAIR: first wave of a pair): lanes 0..31 store one 16-byte piece (row, 8 units)
    const int prow = lane >> 1, phalf = lane & 1;
    const int pu0 = ubase + phalf * 8;
    const bool pk_ok = lane < 32 && prow < nrows && pu0 < Hp;
    const unsigned pbase = pk_ok ? ((unsigned)(dc.b0 + prow) * a.Ypitch + dir * Hp + pu0) * 2u + t0off : szYb;  // out of range: dropped
    const unsigned pstep = pk_ok ? tstep : 0u;

    unsigned char* wl = smem + 2 * ATILE + wave * WAVE_LDS;
    float* patchP = reinterpret_cast<float*>(wl);                    // [GW][256]
    float* patchY = reinterpret_cast<float*>(wl + GW * 1024);        // [256]
    float* patchS = reinterpret_cast<float*>(wl + (GW + 1) * 1024);  // [NSW][256]
    unsigned short* patchB = reinterpret_cast<unsigned short*>(wl + (GW + 1 + NSW) * 1024);  // [16][16] bf16
    unsigned char* xch = smem + XCH + uw * (GW * 1024) + lane * 16;  // PAIR: + gg * 1024
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.Yb, szYb);
    float* trash = a.trash + (tid & 63) * 4;

    // projections of step tt (vector layout; staged to the gate-math layout at the top of that step)
    f32x4 pv[GW];
    auto load_proj = [&](int tt, auto E) {
        const unsigned ts = (unsigned)(dir ? (T - 1 - tt) : tt);
#pragma unroll
        for (int gg = 0; gg < GW; ++gg) pv[gg] = ld4<decltype(E)::value>(Pd, vP0 + ts * vPs + (g0 + gg) * H, vnv);
    };
    // layer output and saved gates of step tt: wave patches -> HBM, 16 bytes per lane.  (a.S == null: a validation /
    // forward chunk - nothing is saved; a.Y == null with it: an inner layer, Yb is its output.)  PAIR: the first wave
    // writes Y and the slots f, i, c (0, 1, 4), the second o, g (2, 3)
    auto flush_outputs = [&](int tt, auto E, auto HALFC) {
        constexpr int EE = decltype(E)::value;
        const unsigned ts = (unsigned)(dir ? (T - 1 - tt) : tt);
        if constexpr (!PAIR) {
            if (a.Y != nullptr) st4<EE>(a.Y, vY0 + ts * vYs, vnv, trash, patch_get_vec(patchY, lane));
            if (a.S != nullptr) {
#pragma unroll
                for (int k = 0; k < NS; ++k) st4<EE>(a.S, vS0 + ts * vSs + k * H, vnv, trash, patch_get_vec(patchS + k * 256, lane));
            }
        } else if constexpr (decltype(HALFC)::value == 0) {
            if (a.Y != nullptr) st4<EE>(a.Y, vY0 + ts * vYs, vnv, trash, patch_get_vec(patchY, lane));
            if (a.S != nullptr) {
                st4<EE>(a.S, vS0 + ts * vSs + 0 * H, vnv, trash, patch_get_vec(patchS, lane));
                st4<EE>(a.S, vS0 + ts * vSs + 1 * H, vnv, trash, patch_get_vec(patchS + 256, lane));
                st4<EE>(a.S, vS0 + ts * vSs + 4 * H, vnv, trash, patch_get_vec(patchS + 512, lane));
            }
        } else if (a.S != nullptr) {
            st4<EE>(a.S, vS0 + ts * vSs + 2 * H, vnv, trash, patch_get_vec(patchS, lane));
            st4<EE>(a.S, vS0 + ts * vSs + 3 * H, vnv, trash, patch_get_vec(patchS + 256, lane));
        }
    };
#define PKD_LP0(E) load_proj(0, E)
    PK_EDGE_DISPATCH(PKD_LP0);
    // self-filling exchange (pk_rec2_common.h): the publishing lanes pattern their own chunks
    const u32x4 sentinel = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (a.self_fill && half == 0) {
        for (int tt = 0; tt < PK_R2_FILL_AHEAD && tt < T; ++tt) pub_store<false>(rs, pbase + (unsigned)tt * pstep, sentinel);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    bool dead = false;
    const bool fast_rt = __builtin_amdgcn_readfirstlane((int)(cluster_on_one_xcd(a, c, p, tid, dead) && a.force_safe == 0)) != 0;
    // the time loop, instantiated per (XCD-local fast path?, static edge case?, which wave of the pair?)
    auto run = [&](auto FASTC, auto SEC, auto HALFC) {
    constexpr bool fast = decltype(FASTC)::value != 0;
    constexpr int SE = decltype(SEC)::value;
    constexpr int HALF = decltype(HALFC)::value;
    for (int t = 0; t < T; ++t) {
        f32x4 acc[GW];
#pragma unroll
        for (int gg = 0; gg < GW; ++gg) acc[gg] = f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned char* At = smem + (t & 1) * ATILE;
        // this step's projections (loaded a step ago) -> the wave's patch, before the poll takes its registers
#pragma unroll
        for (int gg = 0; gg < GW; ++gg) patch_put_vec(patchP + gg * 256, lane, pv[gg]);
        if (t > 0) {
            // (the trash slot is addressed from the start of the LDS whichever A tile is being filled: it stays inside
            // the allocation)
            unsigned goff[NCH];
            int lo[NCH];
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const bool own = clds[i] != LDS_TRASH;
                goff[i] = cbase[i] + (own ? (unsigned)(t - 1) * tstep : 0u);
                lo[i] = clds[i] + (own ? (t & 1) * ATILE : 0);
            }
            // (PAIR: the second wave is done earlier than the first and waits a little longer before it polls)
            const int nap = a.poll_delay + (HALF ? a.helper_delay : 0);
            for (int d = 0; d < nap; ++d) __builtin_amdgcn_s_sleep(1);
            int retries = 0;
            dead = poll_to_lds<NCH, fast>(rs, goff, lo, smem, a.err, a.spin_limit, lane, dead, retries);
        }
        PK_BARRIER_LDS();  // A: the polled h_{t-1} tile is complete
        // off the dependency chain: fp32 outputs of the previous step, projections of the next one, the fill pattern ahead
        if (t > 0) {
#define PKD_FO(E) flush_outputs(t - 1, E, HALFC)
            PK_EDGE_DISPATCH_S(PKD_FO);
        }
        if (t + 1 < T) {
#define PKD_LP1(E) load_proj(t + 1, E)
            PK_EDGE_DISPATCH_S(PKD_LP1);
        }
        if constexpr (HALF == 0) {
            if (a.self_fill && t + PK_R2_FILL_AHEAD < T) pub_store<fast>(rs, pbase + (unsigned)(t + PK_R2_FILL_AHEAD) * pstep, sentinel);
        }
        if (t > 0) {
            const unsigned char* Ar = At + (lane & 15) * (LDA * 2) + kq * 16;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(Ar + kk * 64);
#pragma unroll
                for (int gg = 0; gg < GW; ++gg) acc[gg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, Bf[gg][kk], acc[gg], 0, 0, 0);
            }
        }
        float pre[GW][4];
#pragma unroll
        for (int gg = 0; gg < GW; ++gg) patch_get_cd(patchP + gg * 256, kq, lane, pre[gg]);
        const unsigned poff = pbase + (unsigned)t * pstep;
        if constexpr (!PAIR) {
            // ---- gate math for my (row, unit) pairs: pk_rec_persist2.hip's expressions
            float hv[4], sv[NS][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pr[G];
#pragma unroll
                for (int g = 0; g < G; ++g) pr[g] = pre[g][r] * psc[g] + psh[g] + acc[g][r];
                float h, cc, s[NS];
                pk_cell_fwd<CELL>(act, pr, hprev[r], cprev[r], msk, h, cc, s);
                h = rvf[r] != 0.f ? h : 0.f;  // rows / units outside the layer carry exact zeros (published as padding)
                cc = rvf[r] != 0.f ? cc : 0.f;
                hprev[r] = h;
                cprev[r] = cc;
                hv[r] = h;
#pragma unroll
                for (int k = 0; k < NS; ++k) sv[k][r] = s[k];
                patchB[(kq * 4 + r) * 16 + (lane & 15)] = to_bf_pub(h);
            }
            // ---- publish h_t first: it is what the other workgroups of the cluster wait for
            PK_LDS_ORDER();
            {
                const u32x4 o = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(patchB) + (prow & 15) * 32 + phalf * 16);
                pub_store<fast>(rs, poff, o);
            }
            patch_put_cd(patchY, kq, lane, hv);
#pragma unroll
            for (int k = 0; k < NS; ++k) patch_put_cd(patchS + k * 256, kq, lane, sv[k]);
            PK_LDS_ORDER();
        } else {
            // ---- my two gates (first wave: f, i; second wave: o, g): pk_rec_persist2_lstm.hip's expressions
            float g_a[4], g_b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pa = pre[0][r] * psc[0] + psh[0] + acc[0][r];
                const float pb2 = pre[1][r] * psc[1] + psh[1] + acc[1][r];
                g_a[r] = pk_sig(pa);
                g_b[r] = HALF == 0 ? pk_sig(pb2) : pk_act(act, pb2);
            }
            if constexpr (HALF == 1) {
                *reinterpret_cast<f32x4*>(xch) = f32x4{g_a[0], g_a[1], g_a[2], g_a[3]};
                *reinterpret_cast<f32x4*>(xch + 1024) = f32x4{g_b[0], g_b[1], g_b[2], g_b[3]};
            }
            PK_BARRIER_LDS();  // B: (o, g) of this step are in the pair's hand-over slots
            if constexpr (HALF == 1) {
                patch_put_cd(patchS, kq, lane, g_a);
                patch_put_cd(patchS + 256, kq, lane, g_b);
                PK_LDS_ORDER();
            } else {
                const f32x4 o4 = *reinterpret_cast<const f32x4*>(xch);
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(xch + 1024);
                float hv[4], cv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // neural_networks.py:460-464 with pk_cell_fwd<LSTM>'s expression order.  The contraction is written
                    // out: it is the one the eight-wave kernel of pk_rec_persist2_lstm.hip compiles to (i*g and f*c
                    // rounded, one fused multiply-add with the mask), and this file is built without the packed-fp32
                    // forms, where the compiler would fuse the other product
                    float cc = __builtin_fmaf(g_b[r] * g4[r], msk, g_a[r] * cprev[r]);
                    float h = o4[r] * pk_act(act, cc);
                    h = rvf[r] != 0.f ? h : 0.f;
                    cc = rvf[r] != 0.f ? cc : 0.f;
                    cprev[r] = cc;
                    hv[r] = h;
                    cv[r] = cc;
                    patchB[(kq * 4 + r) * 16 + (lane & 15)] = to_bf_pub(h);
                }
                PK_LDS_ORDER();
                {
                    const u32x4 o = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(patchB) + (prow & 15) * 32 + phalf * 16);
                    pub_store<fast>(rs, poff, o);
                }
                patch_put_cd(patchY, kq, lane, hv);
                patch_put_cd(patchS, kq, lane, g_a);
                patch_put_cd(patchS + 256, kq, lane, g_b);
                patch_put_cd(patchS + 512, kq, lane, cv);
                PK_LDS_ORDER();
            }
        }
    }
    };
    if (half == 0) {
        auto run0 = [&](auto F, auto E) { run(F, E, BoolC<0>()); };
        PK_RUN_SPECIALISED(run0, fast_rt);
#define PKD_FOL0(E) flush_outputs(T - 1, E, BoolC<0>())
        PK_EDGE_DISPATCH(PKD_FOL0);
    } else if constexpr (PAIR) {
        auto run1 = [&](auto F, auto E) { run(F, E, BoolC<1>()); };
        PK_RUN_SPECIALISED(run1, fast_rt);
#define PKD_FOL1(E) flush_outputs(T - 1, E, BoolC<1>())
        PK_EDGE_DISPATCH(PKD_FOL1);
    }
}

// ============================================================================
// backward: dL/dh_{t-1} = direct + [dgates_t] . [U_0; U_1; ...] of the row's direction
// ============================================================================
template <int CELL, int ACT>
__global__ __launch_bounds__(CELL == PK_CELL_LSTM ? 512 : 256, 1) void rec2d_bwd_kernel(R2Args a) {
    const int act = ACT >= 0 ? ACT : a.act;
    constexpr bool PAIR = CELL == PK_CELL_LSTM;
    constexpr int G = pk_cell_gates(CELL), NS = pk_cell_saved(CELL);
    constexpr int NWV = PAIR ? 8 : 4, NT = NWV * 64;
    constexpr int GW = PAIR ? 2 : G;                        // gates of K a wave multiplies
    constexpr int LDA = pk_r2_lda_bf16(G * KPAD);
    constexpr int ATILE = RMAX * LDA * 2;
    constexpr int NBUF = PAIR ? 1 : 2;                      // PAIR: one tile (74 KB), freed by barrier B of the step
    constexpr int NCH = (RMAX * G * (KPAD / 8) + NT - 1) / NT;
    constexpr int NIN = NS + 2 + (PAIR ? 1 : 0);            // saved gates | h_{t-1}, dY (, c_{t-1})
    constexpr int NLD = PAIR ? NIN / 2 : NIN;               // slots a wave loads
    constexpr int GRP_LDS = (NIN + G) * 1024 + G * 512;     // per group of 16 units: inputs | dgate fp32 | dgate bf16
    constexpr int XCH = NBUF * ATILE + 4 * GRP_LDS;         // PAIR: [4 pairs][64 lanes] x 16 bytes of partial dh
    constexpr int LTAB = XCH + (PAIR ? 4 * 1024 : 0);       // PAIR: [NCH][512] LDS byte offsets of the polled chunks
    constexpr int LDS_TRASH = LTAB + (PAIR ? NCH * 512 * 4 : 0);
    constexpr int NPJ = (G * 32 + 63) / 64;                 // 16-byte publish pieces per lane: G gates x 16 rows x 2 halves
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, uw = wave & 3;
    const int half = PAIR ? __builtin_amdgcn_readfirstlane(wave >> 2) : 0;  // PAIR: 0 = gates f, i of K + the gate math; 1 = o, g
    const int g0 = half * GW;
    const int c = blockIdx.x % a.C, p = blockIdx.x / a.C;
    const int H = a.H, Hp = a.Hp, B = a.B, T = a.T, GH = G * H;
    const unsigned TB = (unsigned)T * B;
    const DirCluster dc = dir_cluster(a, c);
    const int dir = dc.dir, nrows = dc.nrows;
    if (nrows <= 0) return;
    const int ubase = p * 64 + uw * 16;
    const int unit = ubase + (lane & 15);
    const bool unit_ok = unit < H;
    const int kq = lane >> 4;
    const float* const Ud = a.U + (size_t)dir * G * H * H;

    // B[kidx = (g, j)][n = unit] = U_g[j][unit], my gates
    bf16x8 Bf[GW][KSTEPS];
    {
        const unsigned szU = (unsigned)((size_t)G * H * H * 4);
        const __amdgpu_buffer_rsrc_t rsU = make_rsrc(Ud, szU);
#pragma unroll
        for (int gg = 0; gg < GW; ++gg)
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) {
                unsigned raw[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int j = kk * 32 + kq * 8 + e;
                    raw[e] = __builtin_amdgcn_raw_buffer_load_b32(
                        rsU, (unit_ok && j < H) ? (unsigned)((((g0 + gg) * H + j) * H + unit) * 4) : szU, 0, 0);
                }
                bf16x8 f;
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (short)pk_f2bf(__uint_as_float(raw[e]));
                Bf[gg][kk] = f;
                if (kk % 3 == 2) {  // fenced in groups of 24 loads
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
    }
    for (int i = tid; i < (LDS_TRASH + 16) / 4; i += NT) reinterpret_cast<unsigned*>(smem)[i] = 0u;

    // ---- poll descriptors: chunk ci = (row, gate, col) of the cluster's dgates_{t+1} block.  Iteration it (t = T-1-it,
    // it >= 1) reads storage time (dir ? it-1 : T-it): goff moves by ONE step for the whole workgroup.  Slots a lane does
    // not own stay out of range (zeros, never the sentinel) and land in the LDS trash slot.
    const int CPR = Hp >> 3;
    const unsigned TS = (unsigned)B * a.Gpitch * 2u;  // bytes per time slab of dGb
    const unsigned szGb = 2u * (unsigned)T * TS;
    const unsigned tstep = dir ? TS : 0u - TS;        // per ITERATION (the steps run T-1, T-2, ...)
    const unsigned slab0 = (unsigned)dir * (unsigned)T * TS + (dir ? 0u : (unsigned)(T - 1) * TS);  // slab of iteration 0
    unsigned goff[NCH], gstep[NCH];
    int clds[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ci = tid + NT * i;
        const bool ok = ci < nrows * G * CPR;
        const int row = ok ? ci / (G * CPR) : 0;
        const int rem = ok ? ci - row * (G * CPR) : 0;
        const int g = rem / CPR, col = rem - g * CPR;
        goff[i] = ok ? slab0 + ((unsigned)(dc.b0 + row) * a.Gpitch + g * Hp + col * 8) * 2u : szGb;
        gstep[i] = ok ? tstep : 0u;
        clds[i] = ok ? row * (LDA * 2) + (g * KPAD + col * 8) * 2 : LDS_TRASH;
    }
    const float msk = a.mask_scalar;
    float rvf[4], dh_dir[4], dc_car[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        rvf[r] = (kq * 4 + r < nrows && unit_ok) ? 1.f : 0.f;
        dh_dir[r] = 0.f;
        dc_car[r] = 0.f;
    }
    const int vrow = lane >> 2, vu0 = ubase + (lane & 3) * 4;
    const int vb = dc.b0 + (vrow < nrows ? vrow : 0);
    int vnv = H - vu0;
    vnv = vnv > 4 ? 4 : (vnv < 0 ? 0 : vnv);
    const int edge = __any(vnv > 0 && vnv < 4) != 0 ? ((H & 1) ? 2 : 1) : 0;
    vnv = vrow < nrows ? vnv : 0;
    const unsigned vY0 = ((unsigned)vb * a.YH + dir * H + vu0), vYs = (unsigned)B * a.YH;
    const unsigned vS0 = (((unsigned)dir * TB + vb) * (NS * H) + vu0), vSs = (unsigned)B * NS * H;
    const unsigned vG0 = (((unsigned)dir * TB + vb) * GH + vu0), vGs = (unsigned)B * GH;
    // ---- publish descriptors (PAIR: first wave): piece idx = (gate, row, half of the 16 units)
    unsigned pbase[NPJ], pstep[NPJ];
    int plds[NPJ];
#pragma unroll
    for (int j = 0; j < NPJ; ++j) {
        const int idx = j * 64 + lane;
        const int g = idx >> 5, prow = (idx >> 1) & 15, phalf = idx & 1;
        const int pu0 = ubase + phalf * 8;
        const bool ok = idx < G * 32 && prow < nrows && pu0 < Hp;
        pbase[j] = ok ? slab0 + ((unsigned)(dc.b0 + prow) * a.Gpitch + g * Hp + pu0) * 2u : szGb;  // out of range: dropped
        pstep[j] = ok ? tstep : 0u;
        plds[j] = (g < G ? g : 0) * 512 + prow * 32 + phalf * 16;
    }

    unsigned char* gl = smem + NBUF * ATILE + uw * GRP_LDS;
    float* patchI = reinterpret_cast<float*>(gl);                // [NIN][256]: S slots, h_{t-1}, dY (, c_{t-1})
    float* patchG = reinterpret_cast<float*>(gl + NIN * 1024);   // [G][256] fp32 gate gradients
    unsigned char* patchB = gl + (NIN + G) * 1024;               // [G][16][16] bf16
    unsigned char* xch = smem + XCH + uw * 1024 + lane * 16;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.dGb, szGb);
    float* trash = a.trash + (tid & 63) * 4;

    // saved tensors of one step in the vector layout.  Steps are loaded in order T-1, T-2, ...: the element offsets of the
    // step to load next are running values (oS into S, oY into Y / dY) that move by one time slab per load.  Slots of
    // patchI: [0..NS) saved gates, NS = h_{t-1}, NS+1 = dY, NS+2 = c_{t-1}; PAIR: the first wave loads f, i, o, g, the
    // second c, h_{t-1}, dY, c_{t-1}
    const unsigned dS = dir ? vSs : 0u - vSs, dYs = dir ? vYs : 0u - vYs;
    unsigned oS = vS0 + (unsigned)(dir ? 0 : T - 1) * vSs, oY = vY0 + (unsigned)(dir ? 0 : T - 1) * vYs;
    f32x4 iv[NLD];
    auto load_step_e = [&](int t, auto E, auto HALFC) {
        constexpr int EE = decltype(E)::value;
        const int nvp = t > 0 ? vnv : 0;  // step t-1 sits one slab further along (nothing there when t == 0)
        if constexpr (!PAIR) {
#pragma unroll
            for (int k = 0; k < NS; ++k) iv[k] = ld4<EE>(a.S, oS + k * H, vnv);
            iv[NS] = ld4<EE>(a.Y, oY + dYs, nvp);
            iv[NS + 1] = ld4<EE>(a.dY, oY, vnv);
            if (t == 0) iv[NS] = f32x4{0.f, 0.f, 0.f, 0.f};  // h_{-1} = 0
        } else if constexpr (decltype(HALFC)::value == 0) {
#pragma unroll
            for (int k = 0; k < NLD; ++k) iv[k] = ld4<EE>(a.S, oS + k * H, vnv);
        } else {
            iv[0] = ld4<EE>(a.S, oS + 4 * H, vnv);
            iv[1] = ld4<EE>(a.Y, oY + dYs, nvp);
            iv[2] = ld4<EE>(a.dY, oY, vnv);
            iv[3] = ld4<EE>(a.S, oS + dS + 4 * H, nvp);
            if (t == 0) {  // h_{-1} = c_{-1} = 0
                iv[1] = f32x4{0.f, 0.f, 0.f, 0.f};
                iv[3] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        oS += dS;
        oY += dYs;
    };
    // fp32 gate gradients of step tt (only when the caller wants them): a wave writes the gates it multiplies
    auto flush_outputs_e = [&](int tt, auto E) {
        const unsigned ts = (unsigned)(dir ? (T - 1 - tt) : tt);
#pragma unroll
        for (int gg = 0; gg < GW; ++gg)
            st4<decltype(E)::value>(a.dP2, vG0 + ts * vGs + (g0 + gg) * H, vnv, trash, patch_get_vec(patchG + (g0 + gg) * 256, lane));
    };
    auto flush_outputs = [&](int tt) {
        if (a.dP2 == nullptr) return;
#define PKD_FOB(E) flush_outputs_e(tt, E)
        PK_EDGE_DISPATCH(PKD_FOB);
    };
    if (half == 0) {
#define PKD_LS0(E) load_step_e(T - 1, E, BoolC<0>())
        PK_EDGE_DISPATCH(PKD_LS0);
    } else {
#define PKD_LS1(E) load_step_e(T - 1, E, BoolC<1>())
        PK_EDGE_DISPATCH(PKD_LS1);
    }
    const u32x4 sentinel = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    auto fill_slab = [&](int it, auto FASTC) {  // my pieces of the slab that iteration `it` will publish
#pragma unroll
        for (int j = 0; j < NPJ; ++j) pub_store<decltype(FASTC)::value != 0>(rs, pbase[j] + (unsigned)it * pstep[j], sentinel);
    };
    if (a.self_fill && half == 0) {  // the first slabs, in place before the handshake lets anyone poll
        for (int k = 0; k < PK_R2_FILL_AHEAD && k < T; ++k) fill_slab(k, BoolC<0>());
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    int* ltab = reinterpret_cast<int*>(smem + LTAB) + tid;
    if constexpr (PAIR) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) ltab[i * 512] = clds[i];
    }

    bool dead = false;
    const bool fast_rt = __builtin_amdgcn_readfirstlane((int)(cluster_on_one_xcd(a, c, p, tid, dead) && a.force_safe == 0)) != 0;
    auto run = [&](auto HALFC) {
    constexpr int HALF = decltype(HALFC)::value;
    const bool fast = fast_rt;
    int it = 0;
    for (int t = T - 1; t >= 0; --t, ++it) {
        f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned char* At = smem + (NBUF == 2 ? (it & 1) * ATILE : 0);
        // this step's saved tensors (loaded a step ago) go to the group's patches BEFORE the poll: their registers are
        // free while the poll holds its chunks
#pragma unroll
        for (int k = 0; k < NLD; ++k) patch_put_vec(patchI + (HALF * NLD + k) * 256, lane, iv[k]);
        if (t < T - 1) {
            const int nap = a.poll_delay + (HALF ? a.helper_delay : 0);
            for (int d = 0; d < nap; ++d) __builtin_amdgcn_s_sleep(1);
            int retries = 0;
            if constexpr (PAIR) {
                dead = fast ? poll_to_lds_tab<NCH, true>(rs, goff, ltab, At, a.err, a.spin_limit, lane, dead, retries)
                            : poll_to_lds_tab<NCH, false>(rs, goff, ltab, At, a.err, a.spin_limit, lane, dead, retries);
            } else {  // (two A tiles: the trash slot is addressed from the start of the LDS, so that it stays inside the allocation)
                int lo[NCH];
#pragma unroll
                for (int i = 0; i < NCH; ++i) lo[i] = clds[i] + (clds[i] != LDS_TRASH ? (it & 1) * ATILE : 0);
                dead = fast ? poll_to_lds<NCH, true>(rs, goff, lo, smem, a.err, a.spin_limit, lane, dead, retries)
                            : poll_to_lds<NCH, false>(rs, goff, lo, smem, a.err, a.spin_limit, lane, dead, retries);
            }
        }
        PK_BARRIER_LDS();  // A: the polled dgates_{t+1} tile and the group's input patches are complete
        // off the dependency chain: fp32 gate gradients of the previous step (if wanted), the fill pattern ahead
        if (t < T - 1) flush_outputs(t + 1);
        if constexpr (HALF == 0) {
            if (a.self_fill && it + PK_R2_FILL_AHEAD < T) {
                if (fast) fill_slab(it + PK_R2_FILL_AHEAD, BoolC<1>());
                else fill_slab(it + PK_R2_FILL_AHEAD, BoolC<0>());
            }
        }
        if (t < T - 1) {
            const unsigned char* Ar = At + (lane & 15) * (LDA * 2) + kq * 16;
#pragma unroll
            for (int gg = 0; gg < GW; ++gg)
#pragma unroll
                for (int kk = 0; kk < KSTEPS; ++kk) {
                    const bf16x8 af = *reinterpret_cast<const bf16x8*>(Ar + ((HALF * GW + gg) * KPAD + kk * 32) * 2);
                    if ((kk & 1) == 0) acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, Bf[gg][kk], acc0, 0, 0, 0);
                    else acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, Bf[gg][kk], acc1, 0, 0, 0);
                }
        }
        // saved tensors of the next step: issued BEHIND the MFMA block, so that their registers are free during it; they
        // have the gate math, the publish and the cluster hand-over to land
        if (t > 0) {
#define PKD_LSN(E) load_step_e(t - 1, E, HALFC)
            PK_EDGE_DISPATCH(PKD_LSN);
        }
        if constexpr (HALF == 1) *reinterpret_cast<f32x4*>(xch) = acc0 + acc1;
        // the gate-math wave reads its inputs before barrier B: they were complete at barrier A
        float sin[NIN][4];
        if constexpr (HALF == 0) {
#pragma unroll
            for (int k = 0; k < NIN; ++k) patch_get_cd(patchI + k * 256, kq, lane, sin[k]);
        }
        if constexpr (PAIR) PK_BARRIER_LDS();  // B: the partial sums are handed over, everybody is done reading the A tile
        if constexpr (HALF == 0) {
            f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PAIR) part = *reinterpret_cast<const f32x4*>(xch);
            float dgv[G][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) s[k] = sin[k][r];
                const float hp = sin[NS][r], dy = sin[NS + 1][r];
                const float cp = PAIR ? sin[NIN - 1][r] : 0.f;
                // (the summation orders of pk_rec_persist2_lstm.hip / pk_rec_persist3.hip)
                const float dh = PAIR ? dy + acc0[r] + acc1[r] + part[r] : dy + dh_dir[r] + acc0[r] + acc1[r];
                float dg[G], dhd, dcp;
                pk_cell_bwd<CELL>(act, s, hp, cp, msk, dh, dc_car[r], dg, dhd, dcp);
                // rows / units outside the layer: exact zeros (select, not multiply: their inputs are arbitrary)
                dh_dir[r] = rvf[r] != 0.f ? dhd : 0.f;
                dc_car[r] = rvf[r] != 0.f ? dcp : 0.f;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float d = rvf[r] != 0.f ? dg[g] : 0.f;
                    dgv[g][r] = d;
                    reinterpret_cast<unsigned short*>(patchB)[g * 256 + (kq * 4 + r) * 16 + (lane & 15)] = to_bf_pub(d);
                }
            }
            PK_LDS_ORDER();
#pragma unroll
            for (int j = 0; j < NPJ; ++j) {
                const u32x4 o = *reinterpret_cast<const u32x4*>(patchB + plds[j]);
                const unsigned off = pbase[j] + (unsigned)it * pstep[j];
                if (fast) pub_store<true>(rs, off, o);
                else pub_store<false>(rs, off, o);
            }
            if (a.dP2 != nullptr) {
#pragma unroll
                for (int g = 0; g < G; ++g) patch_put_cd(patchG + g * 256, kq, lane, dgv[g]);
                PK_LDS_ORDER();
            }
        }
        // next step's poll offsets, behind the publish
        if (t < T - 1) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) goff[i] += gstep[i];
        }
    }
    };
    if (half == 0) run(BoolC<0>());
    else if constexpr (PAIR) run(BoolC<1>());
    __syncthreads();  // PAIR: the second wave of a pair flushes gate gradients the first one wrote
    flush_outputs(0);
}

template <int CELL>
Rec2Kernel pick_fwd(int act) {
    return pk_rec2_pick_act(act, rec2d_fwd_kernel<CELL, PK_ACT_RELU>, rec2d_fwd_kernel<CELL, PK_ACT_TANH>, rec2d_fwd_kernel<CELL, -1>);
}
template <int CELL>
Rec2Kernel pick_bwd(int act) {
    return pk_rec2_pick_act(act, rec2d_bwd_kernel<CELL, PK_ACT_RELU>, rec2d_bwd_kernel<CELL, PK_ACT_TANH>, rec2d_bwd_kernel<CELL, -1>);
}

// the kernel of a pass, its block size and its dynamic LDS (the constants of the kernels above)
struct DirsKernel {
    Rec2Kernel k;
    int threads;
    size_t lds;
};
DirsKernel dirs_kernel(int cell, int act, bool backward) {
    const bool pair = cell == PK_CELL_LSTM;
    const int G = pk_cell_gates(cell), NS = pk_cell_saved(cell), nwv = pair ? 8 : 4, nt = nwv * 64;
    DirsKernel d;
    d.threads = nt;
    if (!backward) {
        const int gw = pair ? 2 : G, nsw = pair ? 3 : NS;
        d.lds = 2 * (size_t)RMAX * pk_r2_lda_bf16(KPAD) * 2 + nwv * ((size_t)(gw + 1 + nsw) * 1024 + 512) + (pair ? 4 * gw * 1024 : 0) + 16;
        d.k = pair ? pick_fwd<PK_CELL_LSTM>(act) : pick_fwd<PK_CELL_RNN>(act);
    } else {
        const int nin = NS + 2 + (pair ? 1 : 0), nch = (RMAX * G * (KPAD / 8) + nt - 1) / nt;
        d.lds = (pair ? 1 : 2) * (size_t)RMAX * pk_r2_lda_bf16(G * KPAD) * 2 + 4 * ((size_t)(nin + G) * 1024 + (size_t)G * 512) +
                (pair ? 4 * 1024 + (size_t)nch * 512 * 4 : 0) + 16;
        d.k = pair ? pick_bwd<PK_CELL_LSTM>(act) : pick_bwd<PK_CELL_RNN>(act);
    }
    return d;
}

// Plan of one launch over both directions (R = 2B rows): the shared-U plan's cluster budget, split evenly; every cluster
// direction-pure.  pl.launches != 1: the shape is not covered (its clusters would not all be resident at once).
int dirs_plan(int R, int H, Plan2& pl) {
    const int rc = pk_rec2_make_plan(R, H, pl);
    if (rc) return rc;
    const int B = R / 2;
    int Cd = pl.C / 2;
    if (pl.launches != 1 || Cd < 1) {
        pl.launches = 2;
        return 0;
    }
    int rpc = (B + Cd - 1) / Cd;
    if (rpc > RMAX) {
        pl.launches = 2;
        return 0;
    }
    Cd = (B + rpc - 1) / rpc;  // (no cluster without rows)
    pl.C = 2 * Cd;
    pl.rpc = rpc;
    return 0;
}

constexpr int NOT_COVERED = 1;  // the entries' "take the one-launch-per-direction path": nothing was launched, no error is set

// cell / variant / shape / residency: 0 = covered
int dirs_covered(int cell, int act, bool backward, int T, int B, int H, Plan2& pl, DirsKernel& dk) {
    if (cell != PK_CELL_LSTM && cell != PK_CELL_RNN) return NOT_COVERED;
    if (cell == PK_CELL_LSTM && !pk_rec2l_enabled()) return NOT_COVERED;  // (the four-wave LSTM of PK_EXPERIMENT lstm_waves)
    if (T <= 0 || B <= 0 || H <= 0 || H > KPAD) return NOT_COVERED;
    if (dirs_plan(2 * B, H, pl) != 0 || pl.launches != 1) return NOT_COVERED;
    dk = dirs_kernel(cell, act, backward);
    // every workgroup of BOTH directions' clusters has to be resident at the same time
    struct Entry { const void* k; int cap; };
    static Entry cache[16];
    static int n_cache = 0;
    int cap = -1;
    for (int i = 0; i < n_cache; ++i)
        if (cache[i].k == (const void*)dk.k) cap = cache[i].cap;
    if (cap < 0) {
        if (pk_grant_dynamic_lds((const void*)dk.k, dk.lds) != 0) return NOT_COVERED;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)dk.k, dk.threads, dk.lds) != hipSuccess) return NOT_COVERED;
        cap = per_cu * pk_num_cu();
        if (n_cache < 16) cache[n_cache++] = Entry{(const void*)dk.k, cap};
    }
    return pl.C * pl.Pn <= cap ? 0 : NOT_COVERED;
}

}  // namespace

// 1 = pk_rec_fwd_bf16_dirs and pk_rec_bwd_bf16_dirs run this layer in one launch each; 0 = one launch per direction
extern "C" int pk_rec_dirs_covered(int cell, int act, int T, int B, int H) {
    Plan2 pl;
    DirsKernel dk;
    return dirs_covered(cell, act, false, T, B, H, pl, dk) == 0 && dirs_covered(cell, act, true, T, B, H, pl, dk) == 0;
}

extern "C" int pk_rec_fwd_bf16_dirs(void* stream, int cell, int act, int T, int B, int bidir, int H, const float* P,
                                    const float* pscale, const float* pshift, const float* U, const float* mask,
                                    float mask_scalar, float* Y, float* S, uint16_t* Yb, int64_t y_pitch, int prefilled) {
    const char* who = "pk_rec_fwd_bf16_dirs";
    PK_REQUIRE(bidir == 1 && mask == nullptr, "%s: both directions (bidir = 1) and no recurrent mask", who);
    Plan2 pl;
    DirsKernel dk;
    if (dirs_covered(cell, act, false, T, B, H, pl, dk) != 0) return NOT_COVERED;
    PK_REQUIRE(Y != nullptr || S == nullptr, "%s: Y may be null only together with S", who);
    hipStream_t st = pk_stream(stream);
    const int Hp = (H + 7) & ~7;
    PK_REQUIRE(y_pitch >= (int64_t)2 * Hp && (y_pitch % 8) == 0 && ((uintptr_t)Yb & 15) == 0,
               "%s: Yb pitch must be a multiple of 8 and hold 2 x %d elements", who, Hp);
    PK_REQUIRE((double)T * B * y_pitch * 2.0 < 4.0e9, "%s: exchange buffer exceeds the 4 GB buffer-descriptor range", who);
    PK_REQUIRE((double)T * B * pk_cell_gates(cell) * H < 4.0e9, "%s: a slab of P exceeds the 32-bit element range", who);
    R2Args a{};
    int rc = pk_rec2_prepare_fwd(a, pl, dirs_plan, cell, act, T, B, 1, H, y_pitch, P, pscale, pshift, U, nullptr, mask_scalar, Y, S);
    if (rc) return rc;
    a.Yb = (unsigned short*)Yb;
    a.self_fill = prefilled == 2 ? 1 : 0;  // (prefilled: see pk_rec_fwd_bf16)
    if (prefilled != 1 && !a.self_fill) PK_CHECK_HIP(hipMemsetAsync(Yb, 0xFF, (size_t)T * B * y_pitch * 2, st));
    if (cell == PK_CELL_LSTM) {
        size_t unused;
        (void)pk_rec2l_kernel(a, act, false, &unused);  // a.helper_delay of the eight-wave kernels (PK_EXPERIMENT lstm_helper_delay)
    }
    // (no L2 run-ahead helpers: pk_rec_helper.hip reads P as one slab)
    return pk_rec2_run(st, a, pl, cell, false, dk.k, dk.threads, dk.lds, who, nullptr, REC2_HELP_NONE);
}

extern "C" int pk_rec_bwd_bf16_dirs(void* stream, int cell, int act, int T, int B, int bidir, int H, const float* U,
                                    const float* mask, float mask_scalar, const float* Y, const float* S, const float* dY,
                                    float* dP2, uint16_t* dGb, int64_t g_pitch, int prefilled) {
    const char* who = "pk_rec_bwd_bf16_dirs";
    PK_REQUIRE(bidir == 1 && mask == nullptr, "%s: both directions (bidir = 1) and no recurrent mask", who);
    Plan2 pl;
    DirsKernel dk;
    if (dirs_covered(cell, act, true, T, B, H, pl, dk) != 0) return NOT_COVERED;
    hipStream_t st = pk_stream(stream);
    const int Hp = (H + 7) & ~7, G = pk_cell_gates(cell);
    PK_REQUIRE(g_pitch >= (int64_t)G * Hp && (g_pitch % 8) == 0 && ((uintptr_t)dGb & 15) == 0,
               "%s: dGb pitch must be a multiple of 8 and hold %d x %d elements", who, G, Hp);
    PK_REQUIRE(2.0 * T * B * g_pitch * 2.0 < 4.0e9, "%s: exchange buffer exceeds the 4 GB buffer-descriptor range", who);
    R2Args a{};
    int rc = pk_rec2_prepare_bwd(a, pl, dirs_plan, cell, act, T, B, 1, H, g_pitch, U, nullptr, mask_scalar, Y, S, dY, dP2);
    if (rc) return rc;
    a.dGb = (unsigned short*)dGb;
    a.self_fill = prefilled == 2 ? 1 : 0;
    if (prefilled != 1 && !a.self_fill) PK_CHECK_HIP(hipMemsetAsync(dGb, 0xFF, (size_t)2 * T * B * g_pitch * 2, st));
    if (cell == PK_CELL_LSTM) {
        size_t unused;
        (void)pk_rec2l_kernel(a, act, true, &unused);
    }
    return pk_rec2_run(st, a, pl, cell, true, dk.k, dk.threads, dk.lds, who, nullptr, REC2_HELP_NONE);
}
