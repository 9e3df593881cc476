// brick_core.hpp — the brick CG apply protocol and the lattice geometry, raw buffer access and patch-buffer
// row sum (patch_sum8) that the brick kernels, the update kernel and the GMRES / BiCGStab passes share.
// The protocol of an apply brick (k_brick_cg of brick_um.hip and of brick_kernels.hip at p <= 2, k_hobrick_cg
// and k_hobrick_um on the p = 3, 4 blocks), and its pieces here:
//   - its place in the lattice: brick_id (XCD order: xcd_order, brick_lattice.hpp), brick_pos -> BrickPos;
//   - the patch gather and d = M^-1 r + beta d_old, stored by the dof's writer brick (is_writer) with the x-fold
//     (each kernel's own loops: they differ in layout and register parking on purpose);
//   - at p = 2, where enabled, the previous update's betanom step (beta_fold);
//   - the element operator (each kernel's own);
//   - the whole patch -> the patch buffer in the pencil layout (patch_store);
//   - the den partial (den_publish, with the grouped tail).
// Both k_brick_cg kernels take brick_pos, is_writer, beta_fold and den_publish; the uniform-box one and
// k_brick3d<PBO> also patch_store.  k_hobrick_cg takes is_writer; otherwise the block kernels still carry
// their own text of steps 1 and 3: which helper costs registers or time at which site is on record in
// profiles/r16/brick_protocol/.  A dof's 1-8 patch entries are summed in one order everywhere (brick_holders
// of brick_lattice.hpp, patch_sum8), which makes the branchy and predicated-load sums bitwise equal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "brick_lattice.hpp"
#include "pa_core.hpp"
#include "reduce.hpp"

#ifndef CDFEM_PS8_SKIP
#define CDFEM_PS8_SKIP 1
#endif

// 1: the uniform-box apply (brick_um.hip) is built for 4 waves per SIMD where its instantiation fits 128
// registers, so that all 16 bricks of a CU are resident at once.  Measured and left at 0 (three waves):
// profiles/r14/ab_c2_one_round/
#ifndef CDFEM_BUM_ONE_ROUND
#define CDFEM_BUM_ONE_ROUND 0
#endif

namespace cdfem {

constexpr bool kUmOneRound = CDFEM_BUM_ONE_ROUND != 0;

struct BrickGeom {
    int nbx, nby, nbz;  // bricks per axis
    int Lx, Ly, Lz;     // dof lattice per axis
    int xcd;            // 1: XCD-contiguous brick order (default; set_option "brick_xcd")
    int bz0, bzs;       // k_brick_cg: the launch covers brick layers bz0, bz0 + bzs, ... (all: 0, 1)
    const uint8_t *bess;  // per brick: 1 if a dof of its patch is essential (nullptr: assume so)
    // first-round stagger of the brick CG apply (k_brick_cg; set_option "brick_stagger"):
    // stag bits 0-3 a shift s, bits 4-8 a count n; stag_round = the workgroups of the first round that may
    // sleep (8 per CU; 16 per CU for the uniform-box apply at 4 waves per SIMD, whose whole C2 launch is one
    // round); stag_min = the smallest launch that staggers (16 per CU: two rounds of 8, one of 16)
    int stag = 0, stag_round = 0, stag_min = 0;
};

// The first round of a brick kernel's workgroups starts together, so every wave gathers its patch at
// once (one HBM burst) and then every wave computes (one VALU crush).  Workgroups b < stag_round with bit
// s of b set (s = log2 CUs: half of every CU's waves) sleep n x 2,048 cycles first, so half the first
// round gathers while the other half computes.  Launches of at least stag_min workgroups only.  C2 (4,096 bricks
// on 256 CUs, n = 4): k_brick_cg 39.0 -> 37.4 us (profiles/r06/ab_c2_stagger/); the GMRES leg's Mult
// (k_brick3d, whose gather is one vector) ran 35.0 -> 35.8 us with it and is left alone.
__device__ __forceinline__ void brick_stagger(const BrickGeom &g)
{
    if (g.stag == 0 || gridDim.x < (unsigned)g.stag_min) return;
    const unsigned wb = blockIdx.x;
    if (wb < (unsigned)g.stag_round && ((wb >> (g.stag & 15)) & 1u))
        for (int i = 0; i < ((g.stag >> 4) & 31); ++i) __builtin_amdgcn_s_sleep(32);
}

// Raw buffer access (MI355X buffer resources): a 32-bit byte offset from a scalar base instead of a
// 64-bit address per lane, and an offset past num_records (kOOB) reads 0 and drops a store, so the
// brick kernels' out-of-lattice positions and predicated stores need neither branches nor clamps.
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
constexpr uint32_t kOOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc(const void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ double bload(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t r, uint32_t off, double v)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, v), r, off, 0, 0);
}

// Patch positions i = t, t + STEP, t + 2 STEP, ... of an S^3 patch (x fastest), advanced incrementally:
// STEP = dz S^2 + dy S + dx, so each step adds (dx, dy, dz) with carries (a few adds and selects
// instead of two constant divisions per position; STEP < S^3)
template <int S, int STEP = 64>
struct PatchWalk {
    int x, y, z;
    __device__ __forceinline__ explicit PatchWalk(unsigned t) : x((int)(t % S)), y((int)((t / S) % S)), z((int)(t / (S * S))) {}
    __device__ __forceinline__ void next()
    {
        constexpr int dx = STEP % S, dy = (STEP / S) % S, dz = STEP / (S * S);
        x += dx;
        const int cx = x >= S ? 1 : 0;
        x -= S & -cx;
        y += dy + cx;
        const int cy = y >= S ? 1 : 0;
        y -= S & -cy;
        z += dz + cy;
    }
};

// the launch-local brick of this workgroup: with xcd = 1 in xcd_order.  Measured in process (tools/ab.py,
// 64^3 p=2, two boxes): 242.8 vs 258.6 us per k_brick_cg launch; at 256^3 no difference (14444 vs 14470 us).
__device__ __forceinline__ int brick_id(const BrickGeom &g)
{
    if (!g.xcd) return blockIdx.x;
    const unsigned G = gridDim.x, b = blockIdx.x;
    return xcd_order(b, G);
}

// Launch-local brick bl -> the global brick b (a launch covers every g.bzs-th layer from g.bz0), its place
// (bx, by, bz) in the brick grid, the lattice origin of its S x S x SZ patch, and whether it is the last brick
// of an axis (which then also writes the dofs of its upper patch face)
struct BrickPos {
    int b, bx, by, bz, gx0, gy0, gz0;
    bool lastx, lasty, lastz;
};
template <int S, int SZ = S>
__device__ __forceinline__ BrickPos brick_pos(const BrickGeom &g, int bl)
{
    const int nxy = g.nbx * g.nby;
    const int bz = g.bz0 + (bl / nxy) * g.bzs;
    const int b = bl % nxy + nxy * bz;
    const int bx = b % g.nbx, by = (b / g.nbx) % g.nby;
    return BrickPos{b, bx, by, bz, (S - 1) * bx, (S - 1) * by, (SZ - 1) * bz,
                    bx == g.nbx - 1, by == g.nby - 1, bz == g.nbz - 1};
}
// every lattice dof has exactly one writer brick: the one holding it below its upper patch faces (in: the
// position lies inside the lattice)
template <int S, int SZ = S>
__device__ __forceinline__ bool is_writer(int px, int py, int pz, bool in, const BrickPos &p)
{
    return in && (px < S - 1 || p.lastx) && (py < S - 1 || p.lasty) && (pz < SZ - 1 || p.lastz);
}

// PatchWalk plus the lattice index gid = gx + Lx gy + Lxy gz of the position, advanced with the walk's
// carries (no per-position 32-bit multiplies: v_mul_lo_u32 issues at a quarter of the VALU rate)
template <int S, int STEP = 64>
struct LatWalk {
    int x, y, z;
    uint32_t gid;
    __device__ __forceinline__ LatWalk(unsigned t, uint32_t g0, uint32_t Lx, uint32_t Lxy)
        : x((int)(t % S)), y((int)((t / S) % S)), z((int)(t / (S * S)))
    {
        gid = g0 + (uint32_t)x + Lx * (uint32_t)y + Lxy * (uint32_t)z;
    }
    __device__ __forceinline__ void next(uint32_t dgid, uint32_t cxd, uint32_t cyd)
    {
        constexpr int dx = STEP % S, dy = (STEP / S) % S, dz = STEP / (S * S);
        x += dx;
        const int cx = x >= S ? 1 : 0;
        x -= S & -cx;
        y += dy + cx;
        const int cy = y >= S ? 1 : 0;
        y -= S & -cy;
        z += dz + cy;
        // dgid = dx + dy Lx + dz Lxy; a carry out of x adds Lx - S, out of y Lxy - S Lx
        gid += dgid + (cxd & (uint32_t)-cx) + (cyd & (uint32_t)-cy);
    }
};

// pa_uniform_diag: the class of lattice coordinate g on an axis of L dofs of a uniform p = 2 box, which with
// the other two axes' classes fixes the assembled diagonal: 0 shared by two elements, 1 element-interior,
// 2 the first plane, 3 the last.  The table index is cx + 4 cy + 16 cz.
__host__ __device__ __forceinline__ int udiag_class(int g, int L) { return g == 0 ? 2 : g == L - 1 ? 3 : g & 1; }

// f(std::integral_constant<int, k>) for k = B .. E - 1, unrolled at compile time (array indices
// stay compile-time, so the arrays stay in registers)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// v unchanged, but opaque to the optimiser: index arithmetic that depends on it cannot be hoisted
// above this point (LLVM otherwise computes a later phase's per-position indices at kernel entry
// and spills them across the element apply)
__device__ __forceinline__ int opaque(int v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// A brick's patch -> the patch buffer pb ([bz][pz][by][py][bx][px], patch_idx in 32-bit arithmetic with the
// brick's part uniform: index = base + pz A + py R + px).  Thread tid of NT stores positions i = tid, tid + NT,
// ... (NI of them, the last only while i < S S SZ) with the entries val(k, i, px, py, pz); what an entry is stays
// in the kernel.  (tid is made opaque: the walk's index arithmetic stays below the element apply.)
template <int S, int SZ = S, int NT = 64, typename F>
__device__ __forceinline__ void patch_store(double *pb, const BrickGeom &g, int bx, int by, int bz, int tid, F &&val)
{
    constexpr int S3 = S * S * SZ, NI = (S3 + NT - 1) / NT;
    const uint32_t R = (uint32_t)g.nbx * S, A = (uint32_t)g.nby * S * R;
    const uint32_t base = (uint32_t)bz * SZ * A + (uint32_t)by * S * R + (uint32_t)bx * S;
    const auto bp = brsrc(pb, 8u * (uint32_t)g.nbx * g.nby * g.nbz * S3);
    const unsigned to = (unsigned)opaque(tid);
    PatchWalk<S, NT> pw(to);
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const unsigned i = to + NT * k;
        if (k == NI - 1 && i >= S3) break;
        bstore(bp, 8u * (base + (uint32_t)pw.z * A + (uint32_t)pw.y * R + (uint32_t)pw.x), val(k, i, pw.x, pw.y, pw.z));
        pw.next();
    }
}

// The den partial of brick b (one wave; t its lane): part[b], and with grouped partials (grp = den_grp > 1)
// the group's sum.  The partial goes out write-through (sc1: an agent-scope relaxed store), the wave waits for
// it, then counts its arrival on the group's agent-scope counter; the brick whose add returns the group's last
// count reads the group's partials with sc1 loads (L2 and L1 bypassed: correct wherever the group's bricks
// ran, MI355X_MICROARCH.md inter-workgroup visibility) and sums them by the fixed wave tree, so the group sum
// does not depend on the order of arrival.  The counter is reset for the next launch by the same brick.
__device__ __forceinline__ void den_publish(double den, int t, int b, double *part, double *gsum, uint32_t *gcnt,
                                            int grp, int nbrick)
{
    den = wave_sum(den);
    if (grp <= 1) {
        if (t == 0) part[b] = den;
        return;
    }
    const int gi = b / grp, g0 = gi * grp, gn = min(grp, nbrick - g0);
    uint32_t prev = 0;
    if (t == 0) {
        __hip_atomic_store(&part[b], den, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        prev = __hip_atomic_fetch_add(&gcnt[gi], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    prev = (uint32_t)__shfl((int)prev, 0, 64);
    if (prev != (uint32_t)(gn - 1)) return;
    double v = t < gn ? __hip_atomic_load(&part[g0 + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    v = wave_sum(v);
    if (t == 0) {
        gsum[gi] = v;
        __hip_atomic_store(&gcnt[gi], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The betanom step of the previous update, taken by the p = 2 apply after kk updates (set_option
// "cg_beta_fold"): betanom from the update's partials pv, which the kernel loaded ahead of its gather (BF 1:
// lane t holds partials t, t + 64, ..., summed in this one order; BF 2: pv[0] is the sum the update's last
// workgroup left), cg_update_logic's decision (cg_stop_kind) taken identically by every workgroup at the
// host's update count kk and recorded by global brick 0 (one launch records, also when a slab is split in
// two), and beta.  True: the solve stops here.
template <int BF, int N>
__device__ __forceinline__ bool beta_fold(const double (&pv)[N], KrylovState *st, int kk, int b, int t, double &beta)
{
    if (kk <= 0) return false;
    double B = pv[0];
    if constexpr (BF == 1) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < N; ++q) v += pv[q];
        B = wave_sum(v);
    }
    const bool stop = cg_stop_kind(st, B, kk) != kCgGoOn;
    if (b == 0 && t == 0) {
#ifdef CDFEM_DEBUG
        assert(st->iter == kk);
#endif
        cg_update_logic_at(st, B, kk);
    }
    if (stop) return true;
    beta = B / st->nom;
    return false;
}

// The 1-8 patch-buffer entries of lattice dof (gx, gy, gz) summed in a fixed order (lower brick first
// per face axis, z outermost): eight buffer loads at fixed offsets from its own brick's entry P (the
// lower brick's face entry along x / y / z sits at P - 1 / P - R / P - A in the pencil layout of
// patch_idx), the absent ones at kOOB (read as 0).  Patches are S x S x SZ (SZ > S: the z-elongated
// high-order blocks, set_option "ho_block_z").
template <int S, int SZ = S>
__device__ __forceinline__ double patch_sum8(__amdgpu_buffer_rsrc_t bp, const BrickGeom &g, int gx, int gy, int gz)
{
    constexpr int s1 = S - 1, sz1 = SZ - 1;
    const int qx = min(gx / s1, g.nbx - 1), qy = min(gy / s1, g.nby - 1), qz = min(gz / sz1, g.nbz - 1);
    const int px = gx - qx * s1, py = gy - qy * s1, pz = gz - qz * sz1;
    const bool fx = px == 0 && qx > 0, fy = py == 0 && qy > 0, fz = pz == 0 && qz > 0;
    const uint32_t R = (uint32_t)g.nbx * S, A = (uint32_t)g.nby * S * R;
    const uint32_t P = (((uint32_t)qz * SZ + pz) * g.nby + qy) * S * R + (uint32_t)py * R + (uint32_t)qx * S + px;
    // (CDFEM_PS8_SKIP: a wave none of whose dofs sits on a y or z brick face issues no load for those
    // neighbours: the 64 consecutive dofs of a wave share one or two lattice rows, so most waves load
    // 2 entries, not 8.  An out-of-range buffer load moves no memory but still returns 64 lanes of
    // data; the skipped terms are the zeros they would have read, so the sum is unchanged)
    bool ax = true, ay = true, az = true;
    if constexpr (CDFEM_PS8_SKIP) {
        ax = __builtin_amdgcn_ballot_w64(fx) != 0;
        ay = __builtin_amdgcn_ballot_w64(fy) != 0;
        az = __builtin_amdgcn_ballot_w64(fz) != 0;
    }
    double t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int sz = (k >> 2) & 1 ? 0 : 1, sy = (k >> 1) & 1 ? 0 : 1, sx = k & 1 ? 0 : 1;
        const bool ok = (!sx || fx) && (!sy || fy) && (!sz || fz);
        const uint32_t o = P - (uint32_t)sx - (uint32_t)sy * R - (uint32_t)sz * A;
        t[k] = 0.0;
        if ((!sx || ax) && (!sy || ay) && (!sz || az)) t[k] = bload(bp, ok ? 8u * o : kOOB);
    }
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) q += t[k];
    return q;
}

// ho_uniform: the 2 x 2 x 4 block CG apply with the dense element matrix (hobrick_um.hip k_hobrick_um), launched
// by the block CG's launcher in place of k_hobrick_cg when ho_uniform_elem(c)
hipError_t launch_hobrick_um(cdfem_ctx *c, const BrickGeom &g, const double *r, const double *dinv, const double *d_old,
                             double *d_new, double *x);

// pa_uniform: the p = 2 brick CG apply with the common element matrix (brick_um.hip k_brick_cg<XF, BF, FULL>),
// launched by brick_cg2_launch in place of the Kronecker-form k_brick_cg when uniform_elem(c): nbrick_launch
// bricks of the layers g.bz0, g.bz0 + g.bzs, ... on stream s (whole: the whole box on the context stream, with
// the profiling events); kk >= 0: the betanom-fold apply after kk updates, with the update's nupart partials
hipError_t launch_brick_um(cdfem_ctx *c, const BrickGeom &g, unsigned nbrick_launch, hipStream_t s, bool whole,
                           const double *r, const double *dinv, const double *d_old, double *d_new, double *x, int kk,
                           int nupart);

// GMRES on the structured Mult (set_option "gm_pb"): A_c V_j is each row's 1-8 patch entries of the
// patch-buffer Mult (k_brick3d<..., PBO>), V_j itself on the essential rows; pass 1 forms it there
// (k_gm_pass1<..., S>), so the E->L kernel's y write and pass 1's re-read of it go away
struct GmPatchSrc {
    const double *pb;    // the patch buffer
    const uint8_t *ess;  // essential flags
    const double *x;     // the Mult's input V_j
    BrickGeom g;
    FastDiv fdx, fdxy;   // lattice row / plane
    int S;               // patch side (4p + 1)
};
// the patch-buffer Mult is in use (brick_mult_pb, Kronecker form, offsets within 32 bits)
bool brick_mult_pb_on(const cdfem_ctx *c);
GmPatchSrc gm_patch_src(const cdfem_ctx *c, const double *x);

}  // namespace cdfem
