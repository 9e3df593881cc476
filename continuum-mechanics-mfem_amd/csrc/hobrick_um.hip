// hobrick_um.hip — ho_uniform: the high-order block CG apply of a uniformly refined box with the common
// element matrix as one dense GEMM on the matrix cores (k_hobrick_um), the uniformity check and the
// element matrix of the PA setup (setup_ho_uniform_elem).  The Kronecker-form kernel it stands in for,
// and the update kernel both share, are in brick_kernels.hip (k_hobrick_cg, k_cg_update_faces).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cdfem_internal.hpp"
#include "brick_core.hpp"
#include "pa_core.hpp"
#include "reduce.hpp"

// waves per SIMD k_hobrick_um is compiled for: 2 (<= 256 VGPRs; it takes 183 at p = 4: one 8-wave workgroup
// per CU) or 4 (<= 128 VGPRs: two workgroups per CU, but 48 registers spill: 4.4 against 3.3 ms per C3 apply,
// profiles/r07/ab_c3_ho_uniform/)
#ifndef CDFEM_HOUM_WAVES
#define CDFEM_HOUM_WAVES 2
#endif

namespace cdfem {

// ================================================================================================
// ho_uniform: the 2 x 2 x 4 block CG apply of a uniform box with the common element matrix as one GEMM
// on the matrix cores.  Steps 1 and 3 are k_hobrick_cg<..., EZ 4>'s; step 2 is
//   Y (N x 16) = A (N x N) X (N x 16),  N = D1^3 (64, 125), one column per element of the block,
// on v_mfma_f64_16x16x4_f64.  The kernel is persistent: wave w of a workgroup holds row tile w of A
// (rows 16 w .. 16 w + 15, KS = ceil(N / 4) k-steps, one double per lane and step: 32 at p = 4) in
// registers for the kernel's life, and the workgroup walks blocks vb = blockIdx, blockIdx + gridDim, ...
// (A is 128 KB at p = 4: re-read per block it would be twice the kernel's HBM bytes of L2 traffic).
// Every block's result depends on the block alone (its patch, its den partial part[b]), so the iterates
// are bitwise the same for any grid.
//   B operand of lane (n = lane & 15, k = lane >> 4) at k-step ks: node 4 ks + k of element n, read from
//   the LDS patch (0 in the k padding and for an element outside the box, whose Y and den term are
//   then exactly 0); accumulator register i of lane (n, k) = row 16 w + 4 i + k of element n.
// amat: [row tile][k step][lane] = A[16 mt + (lane & 15)][4 ks + (lane >> 4)], zero-padded.
// ================================================================================================
template <int D1, bool XF>
__global__ void __launch_bounds__(64 * ((D1 * D1 * D1 + 15) / 16), CDFEM_HOUM_WAVES)
k_hobrick_um(const double *__restrict__ r, const double *__restrict__ dinv, const double *__restrict__ d_old,
             double *__restrict__ d_new, double *__restrict__ face, const double *__restrict__ amat,
             const uint8_t *__restrict__ ess, const BrickGeom g, int nex, int ney, int nez,
             double *__restrict__ part, const KrylovState *__restrict__ st, double *__restrict__ x, int zlo_shared,
             int nblk)
{
    constexpr int P = D1 - 1, EB = kHoBrickEdge, EZ = 4, S = EB * P + 1, SZ = EZ * P + 1, S3 = S * S * SZ;
    constexpr int DD = D1 * D1, ND = DD * D1, NEB = EB * EB * EZ;
    constexpr int NW = (ND + 15) / 16, KS = (ND + 3) / 4, NT = 64 * NW, NI = (S3 + NT - 1) / NT;
    static_assert(NEB == 16, "one block = the 16 columns of one MFMA tile");
    static_assert(KS % 2 == 0, "the B offsets are packed two per register");
    // the patch in LDS with padded row and plane pitches (p = 4: 10 and 92 doubles), so that the 16 elements'
    // corners, 4 lex + 4 SP ley + 4 PP lez doubles apart, spread the B-operand reads over the banks: in units
    // of 4 doubles lex + 2 ley + 4 lez mod 8, every residue twice = the two passes a 64-lane b64 read takes
    constexpr int SP = D1 == 5 ? 10 : S, PP = D1 == 5 ? 92 : S * S;
    static_assert(SP >= S && PP >= S * SP && PP * SZ < 65536, "padded patch");
    __shared__ double s_in[PP * SZ];
    __shared__ double sY[NEB][ND];  // [element][dz][dy][dx]
    __shared__ double shd[NW];
    if (st->done) return;
    const double beta = st->beta;
    const double alpha_prev = XF ? st->alpha : 0.0;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, n16 = lane & 15, kg = lane >> 4;
    const int nxy = g.nbx * g.nby;
    const int Lx = g.Lx, Lxy = g.Lx * g.Ly;
    const uint32_t nl = (uint32_t)Lxy * (uint32_t)g.Lz;
    const auto br = brsrc(r, 8u * nl), bm = brsrc(dinv, 8u * nl), bo = brsrc(d_old, 8u * nl);
    const auto be = brsrc(ess, nl), bd = brsrc(d_new, 8u * nl), bxf = brsrc(x, XF ? 8u * nl : 0u);
    const auto bp = brsrc(face, 8u * (uint32_t)nblk * S3);
    // this wave's row tile of A
    double av[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) av[ks] = amat[((size_t)wv * KS + ks) * 64 + lane];
    // this lane's element (column n16) and the patch offsets of its B operands and accumulator rows
    const int lex = n16 & 1, ley = (n16 >> 1) & 1, lez = n16 >> 2;
    const int ob = P * lez * PP + P * ley * SP + P * lex;
    auto node_off = [&](int j) { return (j / DD) * PP + ((j / D1) % D1) * SP + j % D1; };
    uint32_t jo[KS / 2];
#pragma unroll
    for (int k2 = 0; k2 < KS / 2; ++k2) {
        const int j0 = 8 * k2 + kg, j1 = j0 + 4;
        jo[k2] = (uint32_t)(ob + node_off(j0 < ND ? j0 : 0)) | ((uint32_t)(ob + node_off(j1 < ND ? j1 : 0)) << 16);
    }
    int mo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = 16 * wv + 4 * i + kg;
        mo[i] = ob + node_off(m < ND ? m : 0);
    }
    // blocks in brick_id's order: workgroup w (XCD w % 8) stays inside that XCD's contiguous range
    struct Blk {
        int b, bx, by, bz;
        bool bhas;
    };
    auto blk_of = [&](int vb) {
        const int b = g.xcd ? xcd_order((unsigned)vb, (unsigned)nblk) : vb;
        const int bz = b / nxy, by = (b - bz * nxy) / g.nbx, bx = b - bz * nxy - by * g.nbx;
        return Blk{b, bx, by, bz, g.bess == nullptr || g.bess[b] != 0};
    };
    // the patch loads of a block, all issued before any is consumed (kOOB outside the lattice: 0).  The
    // loads of the workgroup's next block are issued before step 2 of the current one, so their latency
    // runs under its GEMM, E->L sum and stores.
    double rv[NI], mv[NI], ov[NI], xv[NI];
    uint32_t offv[NI];
    uint8_t ev[NI];
    auto gather = [&](const Blk &k) {
        const int gx0 = (S - 1) * k.bx, gy0 = (S - 1) * k.by, gz0 = (SZ - 1) * k.bz;
        const bool lastx = k.bx == g.nbx - 1, lasty = k.by == g.nby - 1, lastz = k.bz == g.nbz - 1;
        PatchWalk<S, NT> pw0(tid);
#pragma unroll
        for (int kk = 0; kk < NI; ++kk) {
            const unsigned i = tid + NT * kk;
            const int px = pw0.x, py = pw0.y, pz = pw0.z;
            pw0.next();
            const int gx = gx0 + px, gy = gy0 + py, gz = gz0 + pz;
            const bool in = i < S3 && gx < g.Lx && gy < g.Ly && gz < g.Lz;
            const uint32_t gid = (uint32_t)opaque(gx + Lx * gy + Lxy * gz);
            offv[kk] = in ? 8u * gid : kOOB;
            rv[kk] = bload(br, offv[kk]);
            mv[kk] = bload(bm, offv[kk]);
            ov[kk] = bload(bo, offv[kk]);
            ev[kk] = 0;
            if (k.bhas) ev[kk] = __builtin_amdgcn_raw_buffer_load_b8(be, in ? gid : kOOB, 0, 0);
            const bool writer = in && (px < S - 1 || lastx) && (py < S - 1 || lasty) && (pz < SZ - 1 || lastz);
            if constexpr (XF) xv[kk] = bload(bxf, writer ? offv[kk] : kOOB);
        }
    };
    Blk cur = blk_of(blockIdx.x);  // (the grid is at most one workgroup per block)
    gather(cur);
    for (int vb = blockIdx.x; vb < nblk; vb += gridDim.x) {
        const int b = cur.b, bx = cur.bx, by = cur.by, bz = cur.bz;
        const int gz0 = (SZ - 1) * bz;
        const bool lastx = bx == g.nbx - 1, lasty = by == g.nby - 1, lastz = bz == g.nbz - 1;
        const bool valid = EB * bx + lex < nex && EB * by + ley < ney && EZ * bz + lez < nez;
        // 1. the patch (k_hobrick_cg step 1) from the loaded values
        double den = 0.0;
        {
            PatchWalk<S, NT> pw1(tid);
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                const unsigned i = tid + NT * k;
                const int px = pw1.x, py = pw1.y, pz = pw1.z;
                pw1.next();
                if (i >= S3) break;
                const bool in = offv[k] != kOOB;
                const double dn = mv[k] * rv[k] + beta * ov[k];  // 0 outside the lattice
                const bool e = ev[k] != 0;
                const bool writer = in && (px < S - 1 || lastx) && (py < S - 1 || lasty) && (pz < SZ - 1 || lastz);
                const uint32_t woff = writer ? offv[k] : kOOB;
                bstore(bd, woff, dn);
                if constexpr (XF) bstore(bxf, woff, xv[k] + alpha_prev * ov[k]);
                den += (writer && e && !(zlo_shared && gz0 + pz == 0)) ? dn * dn : 0.0;
                s_in[px + SP * py + PP * pz] = e ? 0.0 : dn;
            }
        }
        __syncthreads();
        if (vb + (int)gridDim.x < nblk) {  // (workgroup-uniform)
            cur = blk_of(vb + (int)gridDim.x);
            gather(cur);
        }
        // 2. Y = A X: this wave's 16 rows of the 16 elements, one accumulator chain over the KS k-steps
        {
            v4d_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint32_t off = (jo[ks >> 1] >> (16 * (ks & 1))) & 0xffffu;
                double bv = s_in[off];
                if (4 * ks + 3 >= ND) bv = 4 * ks + kg < ND ? bv : 0.0;  // (the k padding)
                bv = valid ? bv : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], bv, acc, 0, 0, 0);
            }
            // d~ . A_e d~ from the accumulator layout, and Y to LDS for the E->L sum
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = 16 * wv + 4 * i + kg;
                if (m < ND) {
                    den += s_in[mo[i]] * acc[i];
                    sY[n16][m] = acc[i];
                }
            }
        }
        __syncthreads();
        // 3. E->L in the block (k_hobrick_cg step 3) -> the patch buffer
        {
            const uint32_t R = (uint32_t)g.nbx * S, A = (uint32_t)g.nby * S * R;
            const uint32_t base = (uint32_t)bz * SZ * A + (uint32_t)by * S * R + (uint32_t)bx * S;
            const unsigned to = (unsigned)opaque(tid);
            PatchWalk<S, NT> pw(to);
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                const unsigned i = to + NT * k;
                if (i >= S3) break;
                const int px = pw.x, py = pw.y, pz = pw.z;
                const int x0 = px < P ? px : P, y0 = py < P ? py : P;
                const bool hx1 = px >= P, hy1 = py >= P;
                const bool hx0 = px <= P, hy0 = py <= P;
                const int x1 = px - P, y1 = py - P;
                int kz = pz / P;
                kz = kz < EZ ? kz : EZ - 1;
                const int zl = pz - kz * P;
                const bool zlow = zl == 0 && kz > 0;
                double sum = 0.0;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
                    const bool okz = cz ? zlow : true;
                    const int ez8 = cz ? kz : (zlow ? kz - 1 : kz), lz = cz ? 0 : (zlow ? P : zl);
                    const bool ok = (cx ? hx1 : hx0) && (cy ? hy1 : hy0) && okz;
                    const int lx = cx ? x1 : x0, ly = cy ? y1 : y0;
                    const double t = sY[cx + 2 * cy + 4 * ez8][ok ? (lz * D1 + ly) * D1 + lx : 0];
                    sum += ok ? t : 0.0;
                }
                bstore(bp, 8u * (base + (uint32_t)pw.z * A + (uint32_t)pw.y * R + (uint32_t)pw.x), sum);
                pw.next();
            }
        }
        const double bs = block_sum(den, shd);
        if (tid == 0) part[b] = bs;
    }
}

// k_hobrick_um's workgroups: set_option "ho_uniform_grid", or what a CU holds at once (CDFEM_HOUM_WAVES per
// SIMD: one workgroup of 8 waves at p = 4, two of 4 waves at p = 3), at most one per block
static int ho_uniform_grid(const cdfem_ctx *c)
{
    const int per_cu = (c->p == 4 ? 2 : 4) * CDFEM_HOUM_WAVES / 4;
    const int want = c->ho_uniform_grid > 0 ? c->ho_uniform_grid : per_cu * (c->ncu > 0 ? c->ncu : 256);
    return std::max(1, std::min(want, c->hb_nblk));
}

template <int D1>
static hipError_t hobrick_um_launch(cdfem_ctx *c, const BrickGeom &g, const double *r, const double *dinv,
                                    const double *d_old, double *d_new, double *x)
{
    constexpr int NT = 64 * ((D1 * D1 * D1 + 15) / 16);
    const dim3 grid((unsigned)ho_uniform_grid(c)), block(NT);
    if (x)
        CDFEM_LAUNCH(c, (k_hobrick_um<D1, true>), grid, block, 0, r, dinv, d_old, d_new, c->d_face.get(), c->d_hoelem.get(), c->d_ess.get(),
                     g, c->sx, c->sy, c->sz, c->d_hbpart.get(), c->d_state.get(), x, c->zlo_shared, c->hb_nblk);
    else
        CDFEM_LAUNCH(c, (k_hobrick_um<D1, false>), grid, block, 0, r, dinv, d_old, d_new, c->d_face.get(), c->d_hoelem.get(), c->d_ess.get(),
                     g, c->sx, c->sy, c->sz, c->d_hbpart.get(), c->d_state.get(), x, c->zlo_shared, c->hb_nblk);
    return hipGetLastError();
}

hipError_t launch_hobrick_um(cdfem_ctx *c, const BrickGeom &g, const double *r, const double *dinv, const double *d_old,
                             double *d_new, double *x)
{
    if (!ho_uniform_elem(c) || c->d_hbpart == nullptr || c->d_face == nullptr) return hipErrorInvalidValue;
    if (c->p == 3) return hobrick_um_launch<4>(c, g, r, dinv, d_old, d_new, x);
    if (c->p == 4) return hobrick_um_launch<5>(c, g, r, dinv, d_old, d_new, x);
    return hipErrorInvalidValue;
}

// ---- ho_uniform: the common element matrix of a uniform p = 3, 4 box (k_hobrick_um) -----------------
// The high-order factors are stored per element (gaff[e nc + k]).  Each component against element 0's, within
// rtol of its own magnitude (a mass factor at h = 1/128 is not judged against the diffusion factor's scale);
// any component further off flags the box as not uniform (plain vector stores of the same value).
__global__ void __launch_bounds__(256)
k_ho_uniform_check(const double *__restrict__ gaff, int64_t ne, int nc, double rtol, double tiny, int *__restrict__ bad)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    bool diff = false;
    for (int k = 0; k < nc; ++k) {
        const double g0 = gaff[k];
        diff |= !(fabs(gaff[e * nc + k] - g0) <= rtol * fmax(fabs(g0), tiny));
    }
    if (diff) *bad = 1;
}

// k_uniform_elem for N = D1^3 up to 125 columns: thread t forms columns t, t + 64, ... one after the other
// (column j = the Kronecker core on e_j with element 0's factors), row-major N x N
template <int D1, int Q1, unsigned K>
__global__ void __launch_bounds__(64)
k_ho_uniform_elem(const double *__restrict__ gaff, const Tab<D1, Q1> T, double *__restrict__ A)
{
    constexpr int N = D1 * D1 * D1, NC = QLayout<K, 3>::nc;
    double g[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) g[k] = gaff[k];
#pragma unroll 1
    for (int j = threadIdx.x; j < N; j += 64) {
        auto xl = [&](int z, int y, int x) { return (z * D1 + y) * D1 + x == j ? 1.0 : 0.0; };
        double Y[D1][D1][D1];
        kron_core<D1, Q1, K>(xl, g, T, Y);
#pragma unroll
        for (int i = 0; i < N; ++i) A[(size_t)i * N + j] = Y[i / (D1 * D1)][(i / D1) % D1][i % D1];
    }
}

template <int D1, int Q1>
static hipError_t ho_uniform_form(cdfem_ctx *c, double *A)
{
    const Tab<D1, Q1> T = make_tab<D1, Q1>(c->rule_op);
    if (c->kinds == 7) hipLaunchKernelGGL((k_ho_uniform_elem<D1, Q1, 7>), dim3(1), dim3(64), 0, c->stream, c->d_qaff, T, A);
    else hipLaunchKernelGGL((k_ho_uniform_elem<D1, Q1, 5>), dim3(1), dim3(64), 0, c->stream, c->d_qaff, T, A);
    return hipGetLastError();
}

hipError_t setup_ho_uniform_elem(cdfem_ctx *c)
{
    c->d_hoelem.reset();
    const int q1 = c->rule_op.q1;
    // the check is taken when the 2 x 2 x 4 block CG of one rank would run on this setup (use_hobrick_cg)
    if (!c->ho_uniform || !c->structured || c->dim != 3 || c->qlay != 1 || c->pa_affine != 2 || c->d_qaff == nullptr ||
        !((c->p == 3 && q1 == 5) || (c->p == 4 && q1 == 6)) || (c->kinds != 7 && c->kinds != 5) || c->ncomp < 1 ||
        !ho_uniform_path(c))
        return hipSuccess;
    c->hoelem_p = c->p;
    c->hoelem_kinds = c->kinds;
    const int nc = c->ncomp, N = c->nd;
    // one scratch allocation: the flag, then the N x N matrix
    DevBuf<double> scratch;
    scratch.alloc((size_t)N * N + 1);
    int *bad = reinterpret_cast<int *>(scratch.get());
    double *A = scratch + 1;
    int hbad = 0;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_ho_uniform_check, dim3((unsigned)((c->ne + 255) / 256)), dim3(256), 0, c->stream, c->d_qaff,
                           (int64_t)c->ne, nc, 1e-14, 1e-300, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    std::vector<double> h((size_t)N * N);
    if (e == hipSuccess && !hbad) {
        e = c->p == 3 ? ho_uniform_form<4, 5>(c, A) : ho_uniform_form<5, 6>(c, A);
        if (e == hipSuccess) e = hipMemcpyAsync(h.data(), A, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) return e;
    if (hbad) return hipSuccess;  // not uniform: the Kronecker form
    // the A operands of v_mfma_f64_16x16x4_f64 in lane order, one row tile per wave of k_hobrick_um:
    // [mt][ks][lane] = A[16 mt + (lane & 15)][4 ks + (lane >> 4)], 0 in the padding
    const int NW = (N + 15) / 16, KS = (N + 3) / 4;
    std::vector<double> op((size_t)NW * KS * 64, 0.0);
    for (int mt = 0; mt < NW; ++mt)
        for (int ks = 0; ks < KS; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int i = 16 * mt + (l & 15), j = 4 * ks + (l >> 4);
                if (i < N && j < N) op[((size_t)mt * KS + ks) * 64 + l] = h[(size_t)i * N + j];
            }
    DevBuf<double> d;
    d.alloc(op.size());
    e = hipMemcpy(d, op.data(), sizeof(double) * op.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    c->d_hoelem = std::move(d);
    return hipSuccess;
}

}  // namespace cdfem
