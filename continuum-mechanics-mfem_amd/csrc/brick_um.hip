// brick_um.hip — pa_uniform: the p = 2 brick CG apply of a uniformly refined box with the common 27 x 27
// element matrix as one GEMM on the matrix cores (k_brick_cg<XF, BF, FULL, UD>, the overload of the Kronecker-form
// kernel in brick_kernels.hip that brick_cg2_launch takes when uniform_elem(c)), the uniformity check and
// the element matrix of the PA setup (setup_uniform_elem), and the class table of the Jacobi scale
// (pa_uniform_diag: setup_uniform_diag, the UD flag of the apply).  The update kernel it feeds is in
// brick_kernels.hip (k_cg_update_faces).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cdfem_internal.hpp"
#include "dispatch.hpp"
#include "brick_core.hpp"
#include "pa_core.hpp"
#include "reduce.hpp"

// the E->L add of an accumulator into the output patch: 0 = explicit read, add, write (two z layers that
// share no position per batch), 1 = one LDS f64 add without return per step.  A/B in
// profiles/r10/ab_c2_brick_um/.
#ifndef CDFEM_BUM_ADD
#define CDFEM_BUM_ADD 0
#endif

namespace cdfem {

// ---- the row order of the element matrix ---------------------------------------------------------
// Accumulator register i of lane (n16, kg) in tile (mt, nt) is row slot 16 mt + 4 i + kg of element
// (n16 & 3, n16 >> 2, nt).  An element's local dof (dx, dy, dz) lands on patch position 2 e + d per axis,
// so two (element, dof) pairs meet on one position only if their dofs agree mod 2 per axis: the 27 dofs
// fall into 8 parity classes of 8 (the corners), 4, 4, 4, 2, 2, 2 and 1 dofs that never meet each other,
// and one dof's 16 elements of a z layer land on 16 different positions.  The 32 slots are 8 groups
// (mt, i) of 4; kUmRow puts one corner and at most three further dofs of pairwise different classes in a
// group, so the 64 lanes of a step (mt, i, nt) add into 64 different positions with no barrier and no
// atomics, and a position's summation order is the program order of the steps.  Slots (kg 0, kg 1) and
// (kg 2, kg 3) pair an even dx + dy + dz with an odd one: the two rows of a 32-lane half then differ by an
// odd number of doubles and do not add to the element origins' own 2-way bank overlap.
// kUmRow[slot] = local dof dx + 3 dy + 9 dz, -1 in the 5 padding slots.
constexpr int kUmSlots = 32, kUmN = 27;
constexpr int kUmRow[kUmSlots] = {0,  1,  4,  3,  2,  7,  22, 5,  6,  19, 10, 21, 8,  25, 16, 23,
                                  18, 9,  12, 13, 20, 11, 14, -1, 24, 15, -1, -1, 26, 17, -1, -1};
constexpr int um_class(int l) { return (l % 3 & 1) | ((l / 3 % 3 & 1) << 1) | ((l / 9 & 1) << 2); }
constexpr bool um_row_order_ok()
{
    int seen[kUmN] = {};
    for (int g = 0; g < kUmSlots / 4; ++g) {
        int cls = 0;
        if (kUmRow[4 * g] < 0 || um_class(kUmRow[4 * g]) != 0) return false;  // a corner first
        for (int k = 0; k < 4; ++k) {
            const int l = kUmRow[4 * g + k];
            if (l < 0) continue;
            if (l >= kUmN || seen[l]++) return false;
            if (cls & (1 << um_class(l))) return false;  // two dofs of one class in a group
            cls |= 1 << um_class(l);
        }
    }
    for (int l = 0; l < kUmN; ++l)
        if (!seen[l]) return false;
    return true;
}
static_assert(um_row_order_ok(), "kUmRow: every dof once, one class once per group of 4 slots");

// offset of slot 4 g + kg's dof in an S = 9 patch (x fastest), -1 for a padding slot: a select over the
// lane's kg of four compile-time constants
template <int G>
__device__ __forceinline__ int um_slot_off(int kg)
{
    constexpr int S = 9;
    auto off = [](int l) constexpr { return l < 0 ? -1 : (l / 9) * S * S + (l / 3 % 3) * S + l % 3; };
    constexpr int o0 = off(kUmRow[4 * G]), o1 = off(kUmRow[4 * G + 1]), o2 = off(kUmRow[4 * G + 2]),
                  o3 = off(kUmRow[4 * G + 3]);
    return kg == 0 ? o0 : kg == 1 ? o1 : kg == 2 ? o2 : o3;
}
template <int G>
constexpr bool um_group_padded() { return kUmRow[4 * G + 1] < 0 || kUmRow[4 * G + 2] < 0 || kUmRow[4 * G + 3] < 0; }

// ================================================================================================
// The brick CG apply (the protocol of k_brick_cg in brick_kernels.hip: patch gather, d = M^{-1} r + beta
// d_old written by the writer brick, x-fold, beta-fold, den partials, essential-row patch entries, the
// patch buffer k_cg_update_faces reads) with the brick's 64 element applies as
//   Y (27 x 64) = A_e (27 x 27) X (27 x 64),
// 2 x 4 tiles of 16 x 16 over 7 k-steps of 4 = 56 v_mfma_f64_16x16x4_f64.  amat is A_e in operand order
// with its rows in kUmRow's: [mt][ks][lane] = A_e[kUmRow[16 mt + (lane & 15)]][4 ks + (lane >> 4)], 0 in
// the padding, 14 doubles per lane held for the whole kernel.  B (lane: input dof 4 ks + (lane >> 4) of
// element 16 nt + (lane & 15)) comes straight from the LDS patch, 0 for an element of a partial brick
// outside the box (its column of Y is then exactly 0).  The E->L sum is taken in the accumulator layout
// (kUmRow above).  LDS is one patch: the input until the last B operand is read, then zeroed and the output.
// den is taken from the assembled patch in the final store loop: sum over (element, dof) of X Y = sum over
// patch positions of in[pos] * out[pos], because every element sharing a position reads the same in[pos]
// (0 on essential and out-of-lattice positions) and a masked element has Y = 0; the lane that formed a
// position's d stores its output, so in[pos] is still at hand (dev[], s_dev) and den is one FMA per position.
// The k order (columns of A_e, B rows) is the dofs' own: consecutive dofs lie an odd number of doubles
// apart (1, 7 or 61), so the two dofs of a 32-lane half already miss each other's banks and the reads
// sit on the 2-way floor of the 16 element origins (2 ex + 18 ey doubles: 12 distinct bank pairs).
// kinds 7 and 5 differ in A_e only.  FULL: every brick's patch lies inside the lattice.
// UD (pa_uniform_diag): dinv is the 64-entry class table of the Jacobi scale, not the vector.  The wave
// copies it to LDS (one load per lane, issued ahead of the gather) with a 1 behind it, and a position reads
// that 1 if essential, else the entry of its class (udiag_class per axis).  A patch coordinate's class
// comes from one scalar word per axis and brick, 2 bits per coordinate: the parity, 2 at coordinate 0 of
// the first brick, 3 at the last lattice plane where the patch holds it.  The gather packs a position's
// table offset into 9 bits, three positions per register.  Positions past the lattice read some finite
// entry and keep d = 0 (r and d_old load 0 there).
// BF: 0 no betanom fold, 1 the fold from the update's partial vector (every workgroup sums it: several
// ranks, and cg_beta_sum 0), 2 from the one sum the update's last workgroup left (cg_beta_sum: one load).
// Residency: the time is memory latency covered by resident waves.  C2 launches 4,096 single-wave
// workgroups on 256 CUs, 16 per CU; at 3 waves per SIMD 12 are resident, so every CU runs a full round and
// then a round of 4.  At 4 waves per SIMD (<= 128 registers, <= 10,240 B of LDS) all 16 are resident at once.
// CDFEM_BUM_ONE_ROUND 1 builds that: um_waves names the instantiations that reach 128 registers without
// scratch (the table forms, those of a partial box's first apply excepted), which then park part of dev[] in
// LDS and, with the partial vector (BF 1), sum it before the gather is issued instead of under it (um_early:
// one more dependent round trip per wave, and the partials' 32 registers are free when the gather's loads go
// out).  Measured: the fourth wave does not pay by the project's rule (profiles/r14/ab_c2_one_round/), so
// the default build keeps the bound of 2 and its 3 waves.  No instantiation of either build uses scratch
// (tests/test_resource_usage.py).
// ================================================================================================
constexpr bool um_early(int BF, bool UD) { return kUmOneRound && BF == 1 && UD; }
constexpr int um_waves(bool XF, int BF, bool FULL, bool UD)
{
    return kUmOneRound && UD && !(BF != 0 && !XF && !FULL) ? 4 : 2;
}

template <bool XF, int BF, bool FULL, bool UD>
__global__ void __launch_bounds__(64, um_waves(XF, BF, FULL, UD))
k_brick_cg(const double *__restrict__ r, const double *__restrict__ dinv, const double *__restrict__ d_old,
           double *__restrict__ d_new, double *__restrict__ face, const double *__restrict__ amat,
           const uint8_t *__restrict__ ess, const BrickGeom g, int zlo_shared, double *__restrict__ part,
           KrylovState *__restrict__ st, double *__restrict__ x, const double *__restrict__ upart, int nupart,
           int kk, double *__restrict__ gsum, uint32_t *__restrict__ gcnt, int grp, int nbrick)
{
    constexpr int P = 2, S = kBrick * P + 1, S2 = S * S, S3 = S * S * S, NDE = kUmN;
    static_assert(S == 9, "um_slot_off is written for the 9^3 patch");
    __shared__ double s_pat[S3];  // the input patch, then (zeroed after the last B operand is read) the output patch
    __shared__ double s_tab[UD ? kUdiagN + 1 : 1];  // the class table, then 1 (what an essential dof takes)
    // 4 waves: the d of a lane's first NST positions wait in LDS for the store loop (slot [k][lane], read back
    // by the lane that wrote it), the rest in registers: 14 registers less across the MFMA block, where the 64
    // accumulator and 28 A registers are live, and LDS stays within a sixteenth of a CU's (9,944 B)
    constexpr int NST = um_waves(XF, BF, FULL, UD) >= 4 ? 7 : 0;
    __shared__ double s_dev[NST ? NST * 64 : 1];
    if (st->done) return;
    brick_stagger(g);
    double beta = st->beta;
    constexpr int NPL = 16;  // BF 1: partials per lane (nupart <= 64 NPL)
    double pv[BF == 1 ? NPL : 1];
    if constexpr (BF == 1) {
        if (kk > 0) {  // (buffer loads: past nupart they read 0, no branch per load)
            const auto bu = brsrc(upart, 8u * (uint32_t)nupart);
#pragma unroll
            for (int i = 0; i < NPL; ++i) pv[i] = bload(bu, 8u * ((uint32_t)threadIdx.x + 64u * i));
        }
    } else if constexpr (BF == 2) {
        // (the update's last workgroup summed its partials in the order below: one load, written before this
        // launch began)
        if (kk > 0) pv[0] = upart[0];
    }
    const double alpha_prev = XF ? st->alpha : 0.0;
    const int t = threadIdx.x;
    const BrickPos pos = brick_pos<S>(g, brick_id(g));
    const int b = pos.b, gx0 = pos.gx0, gy0 = pos.gy0, gz0 = pos.gz0;
    double den = 0.0;
    // patch gather: every load is issued before any is consumed; out-of-lattice positions of partial
    // bricks use kOOB (loads 0, stores dropped); per position the writer's byte offset and one bit of
    // dbits for "writer, and its d^2 counts in den" (as the Kronecker form's gather, brick_kernels.hip)
    constexpr int NI = (S3 + 63) / 64;
    const int Lx = g.Lx, Lxy = g.Lx * g.Ly;
    const uint32_t nl = (uint32_t)Lxy * (uint32_t)g.Lz;
    const auto br = brsrc(r, 8u * nl), bm = brsrc(dinv, UD ? 8u * kUdiagN : 8u * nl), bo = brsrc(d_old, 8u * nl);
    const auto be = brsrc(ess, nl), bd = brsrc(d_new, 8u * nl), bxf = brsrc(x, XF ? 8u * nl : 0u);
    double rv[NI], mv[UD ? 1 : NI], ov[NI], xv[NI];
    uint32_t cw[UD ? (NI + 2) / 3 : 1] = {};  // UD: the positions' table byte offsets, 9 bits each
    uint32_t wx = 0, wy = 0, wz = 0;          // UD: the axes' class words
    if constexpr (UD) {
        // (e: the patch coordinate of the axis' last lattice plane, past the patch in all but the last brick)
        auto axis_word = [](int b0, int e) {
            return 0x4444u | (b0 == 0 ? 2u : 0u) | (e < S ? 3u << (2 * e) : 0u);
        };
        wx = axis_word(pos.bx, g.Lx - 1 - gx0);
        wy = axis_word(pos.by, g.Ly - 1 - gy0);
        wz = axis_word(pos.bz, g.Lz - 1 - gz0);
        mv[0] = bload(bm, 8u * (uint32_t)t);
    }
    uint32_t woffv[NI];
    uint32_t dbits = 0, ebits = 0;
    uint8_t ev[NI];
    double dev[NI];  // the positions' d (each position is formed and stored by the same thread)
    const uint32_t uLx = (uint32_t)Lx, uLxy = (uint32_t)Lxy;
    constexpr uint32_t wdx = 64 % S, wdy = (64 / S) % S, wdz = 64 / (S * S);
    const uint32_t dgid = wdx + wdy * uLx + wdz * uLxy, cxd = uLx - S, cyd = uLxy - S * uLx;
    LatWalk<S> pw0(t, (uint32_t)gx0 + uLx * (uint32_t)gy0 + uLxy * (uint32_t)gz0, uLx, uLxy);
    auto gather = [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const unsigned i = t + 64 * k;
        const int px = pw0.x, py = pw0.y, pz = pw0.z;
        const uint32_t gid = pw0.gid;
        pw0.next(dgid, cxd, cyd);
        const int gz = gz0 + pz;
        const bool in = i < S3 && (FULL || (gx0 + px < g.Lx && gy0 + py < g.Ly && gz < g.Lz));
        const uint32_t off = in ? 8u * gid : kOOB;
        rv[k] = bload(br, off);
        if constexpr (UD) {
            const uint32_t cl = ((wx >> (2 * px)) & 3u) | (((wy >> (2 * py)) & 3u) << 2) | (((wz >> (2 * pz)) & 3u) << 4);
            cw[k / 3] |= cl << (9 * (k % 3) + 3);
            // (packed here, between this step's loads and the next's: left to the scheduler, the twelve
            // steps' coordinates stay live until the form, 36 registers and a wave per SIMD)
            asm volatile("" : "+v"(cw[k / 3]));
        } else {
            mv[k] = bload(bm, off);
        }
        ov[k] = bload(bo, off);
        ev[k] = __builtin_amdgcn_raw_buffer_load_b8(be, in ? gid : kOOB, 0, 0);
        const bool writer = is_writer<S>(px, py, pz, in, pos);
        woffv[k] = writer ? off : kOOB;
        dbits |= (uint32_t)(writer && !(zlo_shared && gz == 0)) << k;
        if constexpr (XF) xv[k] = bload(bxf, woffv[k]);
    };
    auto form = [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const unsigned i = t + 64 * k;
        if (k == NI - 1 && i >= S3) return;
        const bool e = ev[k] != 0;
        double m;
        if constexpr (UD) {
            // (an essential position reads the 1 behind the table: one 32-bit select on the offset instead
            // of a 64-bit select on the value)
            const uint32_t o = e ? 8u * kUdiagN : (cw[k / 3] >> (9 * (k % 3))) & (8u * (kUdiagN - 1));
            m = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(s_tab) + o);
        } else {
            m = mv[k];
        }
        const double dn = m * rv[k] + beta * ov[k];  // 0 outside the lattice
        bstore(bd, woffv[k], dn);
        if constexpr (XF) bstore(bxf, woffv[k], xv[k] + alpha_prev * ov[k]);
        s_pat[i] = e ? 0.0 : dn;
        ebits |= (uint32_t)e << k;
        if constexpr (k < NST) s_dev[64 * k + t] = dn;
        else dev[k] = dn;
    };
    constexpr bool EARLY = um_early(BF, UD);
    if constexpr (BF != 0 && EARLY) {
        if (beta_fold<BF>(pv, st, kk, b, t, beta)) return;
    }
    static_for<0, NI>(gather);
    if constexpr (BF != 0 && !EARLY) {
        if (beta_fold<BF>(pv, st, kk, b, t, beta)) return;
    }
    if constexpr (UD) {
        s_tab[t] = mv[0];
        if (t == 0) s_tab[kUdiagN] = 1.0;
        __syncthreads();
    }
    static_for<0, NI>(form);
    __syncthreads();

    {
        const int n16 = t & 15, kg = t >> 4;
        double av[2][7];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int ks = 0; ks < 7; ++ks) av[mt][ks] = amat[(mt * 7 + ks) * 64 + t];
        // element 16 nt + n16 of the brick: (ex, ey, ez) = (n16 & 3, n16 >> 2, nt); in a partial brick the
        // elements past the box (their far corner outside the lattice) take B = 0
        const int ob0 = P * (n16 >> 2) * S + P * (n16 & 3);
        const bool vxy = FULL || (gx0 + P * (n16 & 3) + P < g.Lx && gy0 + P * (n16 >> 2) + P < g.Ly);
        auto node_off = [&](int j) { return (j / 9) * S2 + ((j / 3) % 3) * S + j % 3; };
        v4d_t acc[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = v4d_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 7; ++ks) {
            const int j = 4 * ks + kg;  // this lane's input dof (27 = the k padding: B = 0)
            const int jo = node_off(j < NDE ? j : 0);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const bool ok = j < NDE && vxy && (FULL || gz0 + P * nt + P < g.Lz);
                const double xin = s_pat[P * nt * S2 + ob0 + jo];
                const double bv = ok ? xin : 0.0;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt][ks], bv, acc[mt][nt], 0, 0, 0);
            }
        }
        // every B operand is read: the patch is zeroed (each lane its own positions) and takes the output
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NI; ++k)
            if (k < NI - 1 || t + 64 * k < S3) s_pat[t + 64 * k] = 0.0;
        __syncthreads();
        // the E->L sum in the accumulator layout: group G = 4 mt + i, this lane's dof of it at patch offset so
        // (-1: a padding slot, whose Y is 0)
        static_for<0, 8>([&](auto gc) {
            constexpr int G = decltype(gc)::value, mt = G / 4, i = G % 4;
            constexpr bool PADG = um_group_padded<G>();
            const int so = um_slot_off<G>(kg);
            const bool live = !PADG || so >= 0;
            const int o = ob0 + (PADG ? max(so, 0) : so);
            if (live) {
#if CDFEM_BUM_ADD == 1
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    (void)__hip_atomic_fetch_add(&s_pat[P * nt * S2 + o], acc[mt][nt][i], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
#else
                // layers nt and nt + 2 share no position (z = 2 nt + dz): two reads in flight per batch
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    double *const p0 = &s_pat[P * h * S2 + o], *const p1 = &s_pat[P * (h + 2) * S2 + o];
                    const double v0 = *p0, v1 = *p1;
                    *p0 = v0 + acc[mt][h][i];
                    *p1 = v1 + acc[mt][h + 2][i];
                }
#endif
            }
        });
    }
    __syncthreads();

    // the brick's whole patch output (interior rows complete, face rows partial; the essential rows carry
    // the writer's d) -> the patch buffer (patch_store)
    patch_store<S>(face, g, pos.bx, pos.by, pos.bz, t, [&](int k, unsigned i, int, int, int) {
        // an essential row's entry is (A_c d)_i = d_i from its writer (where it counts in den), 0 from the
        // other bricks; den = sum over positions of d~ y (d~ = 0 on essential rows: every element sharing
        // a position read the same d~, and masked elements have y = 0) + the writers' d^2 on essential rows:
        // with the entry formed first, both are d times the entry
        double v = s_pat[i];
        const double dk = k < NST ? s_dev[i] : dev[k];  // (i = 64 k + lane)
        const double dw = ((dbits >> k) & 1u) ? dk : 0.0;
        v = ((ebits >> k) & 1u) ? dw : v;
        den += dk * v;
        return v;
    });
    den_publish(den, t, b, part, gsum, gcnt, grp, nbrick);
}

hipError_t launch_brick_um(cdfem_ctx *c, const BrickGeom &g, unsigned nbrick_launch, hipStream_t s, bool whole,
                           const double *r, const double *dinv, const double *d_old, double *d_new, double *x, int kk,
                           int nupart)
{
    if (c->d_uelem == nullptr || c->p != 2) return hipErrorInvalidValue;
    const dim3 grid(nbrick_launch), block(64);
    const double *upart = c->d_part + c->nblk;                  // the den-fold update's partials
    double *const dpart = c->den_out ? c->den_out : c->d_part;  // the apply's den partials
    const bool full = c->sx % kBrick == 0 && c->sy % kBrick == 0 && c->sz % kBrick == 0;
    // the Jacobi scale from the class table (not under pc = none, whose dinv is the ones vector)
    const bool ud = uniform_diag(c) && dinv == c->d_dinv;
    if (ud) dinv = c->d_udiag;
    // the betanom fold: 1 from the update's partials, 2 from their one sum (cg_beta_sum)
    const bool bs = kk >= 0 && cg_beta_sum_on(c);
    if (bs) upart = c->d_bsum;
    dispatch_value<0, 1, 2>(kk < 0 ? 0 : bs ? 2 : 1, 0, [&](auto BF) {
        dispatch_bools(x != nullptr, full, ud, [&](auto XF, auto FU, auto UD) {
            const auto kern = k_brick_cg<XF(), BF(), FU(), UD()>;
            CDFEM_LAUNCH_ON(c, whole, s, kern, grid, block, 0, r, dinv, d_old, d_new, c->d_face.get(), c->d_uelem.get(), c->d_ess.get(),
                            g, c->zlo_shared, dpart, c->d_state.get(), x, upart, nupart, kk, c->d_gsum.get(), c->d_gcnt.get(), c->den_grp,
                            c->nblk);
        });
        return 0;
    });
    return hipGetLastError();
}

// ---- pa_uniform: the common element matrix of a uniformly refined box ----------------------------
// Every element slot's factors against slot 0's (brick 0, lane 0: element (0, 0, 0)); any component
// further than tol flags the box as not uniform (plain vector stores of the same value).
__global__ void __launch_bounds__(256)
k_uniform_check(const double *__restrict__ gaff, const int32_t *__restrict__ perm, int nslots, int nc, int ne,
                double tol, int *__restrict__ bad)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int e = perm[s];
    if (e < 0 || e >= ne) return;
    const size_t b = (size_t)(s / kLanes), lane = (size_t)(s % kLanes);
    bool diff = false;
    for (int k = 0; k < nc; ++k) diff |= fabs(gaff[(b * nc + k) * kLanes + lane] - gaff[(size_t)k * kLanes]) > tol;
    if (diff) *bad = 1;
}

// column j of the element matrix = the Kronecker core (what k_brick_cg<..., AF 2> applies) on the unit
// vector e_j with element 0's factors: thread j writes A[i][j], row-major N x N
template <int D1, int Q1, unsigned K>
__global__ void __launch_bounds__(64)
k_uniform_elem(const double *__restrict__ gaff, const Tab<D1, Q1> T, double *__restrict__ A)
{
    constexpr int N = D1 * D1 * D1;
    const int j = threadIdx.x;
    if (j >= N) return;
    double g[QLayout<K, 3>::nc];
    kron_load_g<K>(gaff, 0, g);
    auto xl = [&](int z, int y, int x) { return (z * D1 + y) * D1 + x == j ? 1.0 : 0.0; };
    double Y[D1][D1][D1];
    kron_core<D1, Q1, K>(xl, g, T, Y);
    for (int i = 0; i < N; ++i) A[i * N + j] = Y[i / (D1 * D1)][(i / D1) % D1][i % D1];
}

hipError_t setup_uniform_elem(cdfem_ctx *c)
{
    c->d_uelem.reset();
    if (!c->pa_uniform || !c->structured || c->qlay != 0 || c->dim != 3 || pa_af(c) != 2 || c->p != 2 ||
        c->rule_op.q1 != 4 || c->ncomp < 1 || (c->kinds != 7 && c->kinds != 5))
        return hipSuccess;
    const int nc = c->ncomp;
    std::vector<double> g0(nc);
    hipError_t e = hipMemcpy2D(g0.data(), sizeof(double), c->d_qaff, kLanes * sizeof(double), sizeof(double), nc,
                               hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    double gmax = 0.0;
    for (double v : g0) gmax = std::max(gmax, std::fabs(v));
    // one scratch allocation: the flag, then the N x N matrix
    constexpr int N = kUmN;
    DevBuf<double> scratch;
    scratch.alloc(N * N + 1);
    int *bad = reinterpret_cast<int *>(scratch.get());
    double *A = scratch + 1;
    int hbad = 0;
    const int nslots = c->nblk * kLanes;
    e = hipMemsetAsync(bad, 0, sizeof(int), c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_uniform_check, dim3((nslots + 255) / 256), dim3(256), 0, c->stream, c->d_qaff, c->d_perm,
                           nslots, nc, (int)c->ne, 1e-14 * gmax, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    std::vector<double> h(N * N), op(2 * 7 * 64, 0.0);
    if (e == hipSuccess && !hbad) {
        const Tab<3, 4> T = make_tab<3, 4>(c->rule_op);
        if (c->kinds == 7) hipLaunchKernelGGL((k_uniform_elem<3, 4, 7>), dim3(1), dim3(64), 0, c->stream, c->d_qaff, T, A);
        else hipLaunchKernelGGL((k_uniform_elem<3, 4, 5>), dim3(1), dim3(64), 0, c->stream, c->d_qaff, T, A);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h.data(), A, sizeof(double) * N * N, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) return e;
    if (hbad) return hipSuccess;  // not uniform: the Kronecker form
    // the A operands of v_mfma_f64_16x16x4_f64 in lane order, rows in kUmRow's order:
    // [mt][ks][lane] = A[kUmRow[16 mt + (lane & 15)]][4 ks + (lane >> 4)]
    for (int mt = 0; mt < 2; ++mt)
        for (int ks = 0; ks < 7; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int i = kUmRow[16 * mt + (l & 15)], j = 4 * ks + (l >> 4);
                op[(mt * 7 + ks) * 64 + l] = (i >= 0 && j < N) ? h[i * N + j] : 0.0;
            }
    DevBuf<double> d;
    d.alloc(op.size());
    e = hipMemcpy(d, op.data(), sizeof(double) * op.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    c->d_uelem = std::move(d);
    return hipSuccess;
}

// ---- pa_uniform_diag: the Jacobi scale of a uniform box as 64 class values ------------------------
__device__ __forceinline__ int udiag_index(int gid, int Lx, int Ly, int Lz)
{
    const int gx = gid % Lx, gy = (gid / Lx) % Ly, gz = gid / (Lx * Ly);
    return udiag_class(gx, Lx) + 4 * udiag_class(gy, Ly) + 16 * udiag_class(gz, Lz);
}

// first[class] = the lowest lattice index among the class's non-essential dofs (first = ~0 on entry): a
// minimum per workgroup in LDS, then one global atomic minimum per class the workgroup met
__global__ void __launch_bounds__(256)
k_udiag_first(const uint8_t *__restrict__ ess, int Lx, int Ly, int Lz, uint32_t *__restrict__ first)
{
    __shared__ uint32_t lo[kUdiagN];
    if (threadIdx.x < kUdiagN) lo[threadIdx.x] = ~0u;
    __syncthreads();
    const int n = Lx * Ly * Lz;
    for (int gid = blockIdx.x * blockDim.x + threadIdx.x; gid < n; gid += gridDim.x * blockDim.x)
        if (!ess[gid]) atomicMin(&lo[udiag_index(gid, Lx, Ly, Lz)], (uint32_t)gid);
    __syncthreads();
    if (threadIdx.x < kUdiagN && lo[threadIdx.x] != ~0u) atomicMin(&first[threadIdx.x], lo[threadIdx.x]);
}

// the table (1 for a class without a non-essential dof: any finite value serves), one workgroup of 64
__global__ void __launch_bounds__(kUdiagN)
k_udiag_fill(const double *__restrict__ dinv, const uint32_t *__restrict__ first, double *__restrict__ tab)
{
    const uint32_t f = first[threadIdx.x];
    tab[threadIdx.x] = f != ~0u ? dinv[f] : 1.0;
}

// flags[0]: an entry of dinv is not what the kernels would take in its place (1 on an essential dof, else
// within tol, relative, of the class entry); flags[1]: some non-essential entry differs from its class
// entry at all (plain vector stores of the same value)
__global__ void __launch_bounds__(256)
k_udiag_check(const double *__restrict__ dinv, const uint8_t *__restrict__ ess, const double *__restrict__ tab,
              int Lx, int Ly, int Lz, double tol, int *__restrict__ flags)
{
    const int n = Lx * Ly * Lz;
    bool bad = false, inexact = false;
    for (int gid = blockIdx.x * blockDim.x + threadIdx.x; gid < n; gid += gridDim.x * blockDim.x) {
        const double m = dinv[gid];
        if (ess[gid]) {
            bad |= m != 1.0;
        } else {
            const double tv = tab[udiag_index(gid, Lx, Ly, Lz)];
            bad |= !(fabs(m - tv) <= tol * fabs(tv));
            inexact |= m != tv;
        }
    }
    if (bad) flags[0] = 1;
    if (inexact) flags[1] = 1;
}

hipError_t setup_uniform_diag(cdfem_ctx *c)
{
    hipError_t e = hipSuccess;
    c->d_udiag.reset();
    c->udiag_bitwise = false;
    if (c->d_uelem == nullptr || !c->structured || c->dim != 3 || c->p != 2 || c->perm_space ||
        c->nl != c->Lx * c->Ly * c->Lz || c->nl >= ((int64_t)1 << 31))
        return hipSuccess;
    // one allocation: the table, the classes' first indices, the two flags
    DevBuf<double> buf;
    buf.alloc(kUdiagN + (kUdiagN + 2 + 1) / 2);  // (the 32-bit words rounded up to whole doubles)
    double *tab = buf;
    uint32_t *first = reinterpret_cast<uint32_t *>(tab + kUdiagN);
    int *flags = reinterpret_cast<int *>(first + kUdiagN);
    int hflags[2] = {1, 1};
    const int Lx = (int)c->Lx, Ly = (int)c->Ly, Lz = (int)c->Lz;
    const dim3 grid((unsigned)std::min<int64_t>((c->nl + 255) / 256, 1024)), block(256);
    e = hipMemsetAsync(first, 0xff, sizeof(uint32_t) * kUdiagN, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, 2 * sizeof(int), c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_udiag_first, grid, block, 0, c->stream, c->d_ess, Lx, Ly, Lz, first);
        hipLaunchKernelGGL(k_udiag_fill, dim3(1), dim3(kUdiagN), 0, c->stream, c->d_dinv, first, tab);
        hipLaunchKernelGGL(k_udiag_check, grid, block, 0, c->stream, c->d_dinv, c->d_ess, tab, Lx, Ly, Lz, 1e-14, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || hflags[0]) return e;  // not class-constant: the solve streams the vector
    c->d_udiag = std::move(buf);
    c->udiag_bitwise = hflags[1] == 0;
    return hipSuccess;
}

}  // namespace cdfem
