// model.hip — the cost model behind cdfem_kernel_name / cdfem_kernel_flops / cdfem_kernel_bytes: which
// kernel a kernel id runs as in the current configuration, and the flops and bytes one launch of it is
// counted at (the roofline coordinates of bench.py).  Host arithmetic only.
#include <cstdio>

#include "cdfem_internal.hpp"
#include "host_util.hpp"
#include "brick_core.hpp"

namespace cdfem {

// name of the HIP kernel that kernel id runs as in the current configuration (rocprof's kernel
// name without its template arguments): the apply of a CG solve (the roofline kernel of the bench)
void kernel_name(const cdfem_ctx *c, int k, char *buf, size_t n)
{
    if (k == CDFEM_K_UPDATE && c->last_method == CDFEM_BICGSTAB) {
        // the last BiCGStab solve's operator source: the Mult's output (S=0) or the patch buffer (S=4p+1)
        std::snprintf(buf, n, "k_bcgs_v<S=%d>", c->bcgs_src);
        return;
    }
    if (k != CDFEM_K_APPLY) throw UnsupportedError("kernel names: the operator apply only");
    const char *name = nl_jac_current(c) ? "k_nl_tensor"
                       : c->fa_ready ? (c->lds_rows > 0 ? "k_sell_spmv_lds" : "k_sell_spmv")
                       : use_brick(c) ? "k_brick_cg"
                       : ho_uniform_elem(c) ? "k_hobrick_um"
                       : use_hobrick_cg(c) ? "k_hobrick_cg"
                       : c->qlay == 1 ? (tile_kron(c) ? "k_apply3d_ktile" : "k_apply3d_tile")
                                      : "k_apply3d";
    std::snprintf(buf, n, "%s", name);
}

// one k_nl_tensor launch in the Jacobian mode (nl_tensor.hip), per element, FMA = 2.  Fields: u, u - u(dof 0),
// u - u_old and v.  Per thread (Q^2 of them): the x / y contractions of every dz plane (4 field sums and 2
// derivative sums over dx, 8 accumulations per dy), the column's geometry, then per z point the z contraction
// (11 sums over dz), the point (J from the column's faces, adj(J), det J, the two fluxes, the coefficients)
// and the transposed z contraction (4 FMAs per dz); then per local dof the transposed x / y contraction.
static double nl_jvp_flops(const cdfem_ctx *c)
{
    const double D = c->d1, Q = c->heat.rule.q1;
    const bool d3 = c->dim == 3;
    const double DZ = d3 ? D : 1.0, QZ = d3 ? Q : 1.0;
    const double xy = DZ * D * (2.0 * 6 * D + 2.0 * 8 + D);            // (+ the D differences u - u(dof 0))
    const double geo = d3 ? 2 * 3 * (2 + 6 + 8) + 3.0 : 2 * (2 + 6);
    const double zc = 2.0 * (d3 ? 11 : 0) * DZ;
    const double pt = d3 ? (12 * 2 + 27 + 5) + 2 * (2 * 18 + 3) + 30 : (4 + 3) + 2 * (2 * 8 + 2) + 24;
    const double zt = 2.0 * (d3 ? 4 : 3) * DZ;
    const double out = D * D * DZ * Q * (Q * 2.0 * 3 + 2.0 * 2);
    return (Q * Q * (xy + geo + QZ * (zc + pt + zt)) + out) * (double)c->ne;
}

double kernel_flops(const cdfem_ctx *c, int k)
{
    if (k == CDFEM_K_APPLY && nl_jac_current(c)) return nl_jvp_flops(c);
    if (k != CDFEM_K_APPLY || c->fa_ready || c->dim != 3)
        throw UnsupportedError("kernel flops: the 3D partial-assembly apply only");
    // sum factorization, one element (pa_core.hpp elem_apply3d): per z plane the z contraction
    // (D^3 FMA per field), per (z, y) the y contraction, per point the x contraction, the
    // point operator and the transposed x contraction, then the transposed y and z contractions.
    // Fields: value, plus the three reference derivatives when diffusion or convection is on.
    const int D = c->d1, Q = c->rule_op.q1;
    const bool kD = c->kinds & CDFEM_DIFFUSION, kC = c->kinds & CDFEM_CONVECTION, kM = c->kinds & CDFEM_MASS;
    if ((c->qlay == 0 && uniform_elem(c) && use_brick(c)) || (c->qlay == 1 && ho_uniform_elem(c))) {
        // the common element matrix (brick_um.hip k_brick_cg<XF, BF, FULL>, hobrick_um.hip k_hobrick_um): nd^2
        // MACs per element (the MFMA tiles' zero padding is not counted: 56 x 1024 MACs per 64 elements
        // against 64 x 729 at p = 2, 128 x 128 per element at p = 4)
        return 2.0 * (double)c->nd * c->nd * (double)c->ne;
    }
    if ((c->qlay == 0 && pa_af(c) == 2) || (c->qlay == 1 && tile_kron(c))) {
        // Kronecker form (pa_core.hpp elem_apply3d_kron; the tile kernel k_apply3d_ktile runs the
        // same stages across threads), per input z plane: a length-n linear combination counts
        // 2n - 1 flops, an accumulation into Y 2 per term
        const bool kG = kD || kC;
        auto lc = [](int n) { return n > 0 ? 2.0 * n - 1.0 : 0.0; };
        const double x_row = lc(D) * (1 + 2 * kD + kG) + lc(kM + kD + kC) + 2 * lc(kD + kC);
        double y_pt = lc(D) + (kG ? 2 * lc(D) + 1 : 0.0);
        if (kD) y_pt += 6 * lc(D) + 2 + 2 + 1 + 2 + 3;
        const double z_pt = 2.0 * (1 + 2 * kD + kG) * D;
        return (double)D * ((double)D * D * x_row + (double)D * D * (y_pt + z_pt)) * (double)c->ne;
    }
    const int g = (kD || kC) ? 1 : 0;
    double pt_fma = D * (1 + 3 * g) + D * (kD ? 4 : 1), pt_mul = 0.0;  // x contraction, transposed x
    if (kD) { pt_fma += 6; pt_mul += 3; }
    if (kC) { pt_fma += 2; pt_mul += 1; }
    if (kM) { if (kC) pt_fma += 1; else pt_mul += 1; }
    if (c->qlay == 1 ? tile_affine(c) : c->d_qaff != nullptr)
        pt_mul += c->ncomp + 2;  // point data W_q * g_k, W_q = (w_x w_y) w_z
    // pa_geom, ho_geom: the point operator of elem_apply3d<..., GEO> instead of the one above: two columns
    // of J (6 FMA), adj(J) (a mul and an FMA per entry; its first row alone without diffusion and
    // convection), det J (1 mul, 2 FMA), W_q (wq_mul: what of (w_x w_y) w_z is left to the point);
    // t = adj(J)^T grad u (3 mul, 6 FMA); D: W kappa / det J (2 mul, the reciprocal counted as 1 division),
    // the scaled t (3 mul), adj(J) t (3 mul, 6 FMA); C: W (alpha c . t) (2 mul, 2 FMA); M: W s det J
    // (2 mul) and its product with u (an FMA after C, else a mul)
    auto geom_point = [&](int wq_mul) {
        const int na = g ? 9 : 3;
        pt_fma = D * (1 + 3 * g) + D * (kD ? 4 : 1);
        pt_mul = 0.0;
        pt_fma += 6 + na + 2 + (g ? 6 : 0) + (kD ? 6 : 0) + (kC ? 2 : 0) + ((kM && kC) ? 1 : 0);
        pt_mul += na + 1 + wq_mul + (g ? 3 : 0) + (kD ? 2 + 1 + 3 + 3 : 0) + (kC ? 2 : 0) + (kM ? 2 : 0) +
                  ((kM && !kC) ? 1 : 0);
    };
    double geo_fma = 0.0, geo_mul = 0.0;
    if (c->qlay == 0 && pa_geom_on(c)) {
        geom_point(2);  // W_q in full
        geo_fma = (double)Q * (9 + 9 * Q);  // the hoisted parts of J, 9 FMAs per (z, y) and 9 per z plane
    }
    if (c->qlay == 1 && ho_geom_on(c)) {
        // k_apply3d_tile<..., MF 32>: the same point operator with the tile's hoisting.  Per point 32 FMAs
        // and 27 multiplications on top of the contractions at kinds 7, W_q = (w_x w_y) w_z being 1 mul.
        // Per column of points (thread), once: a1 + eta a4, a5 + eta a7, a2 + xi a4, a6 + xi a7
        // (12 FMA), dx/dzeta (6 FMA), w_x w_y (1 mul).
        geom_point(1);
        geo_fma = (double)Q * Q * 18;
        geo_mul = (double)Q * Q;
    }
    const double fma = Q * ((double)D * D * D * (1 + g) + Q * ((double)D * D * (1 + 2 * g) + Q * pt_fma +
                                                               (double)D * D * (kD ? 3 : 1)) +
                            (double)D * D * D * (kD ? 2 : 1)) + geo_fma;
    const double mul = (double)Q * Q * Q * pt_mul + geo_mul;
    return (2.0 * fma + mul) * (double)c->ne;
}

double kernel_bytes(const cdfem_ctx *c, int k)
{
    const double nl = (double)c->nl, ne = (double)c->ne, nd = c->nd;
    if (k == CDFEM_K_APPLY && nl_jac_current(c))
        // the matrix-free Jacobian: u, u_old and v gathered (each L-dof once), the element map, the slot
        // permutation, the vertices, the E-vector write; no point data
        return 24.0 * nl + 4.0 * nd * ne + 4.0 * ne + 8.0 * c->nv * c->dim * ne + 8.0 * nd * ne;
    if (k == CDFEM_K_UPDATE && c->last_method == CDFEM_BICGSTAB) {
        // the five vector kernels of one BiCGStab iteration (bicgstab.hip): k_bcgs_p 4 N, k_bcgs_s 3 N,
        // k_bcgs_x 7 N doubles; k_bcgs_v and k_bcgs_t each write their vector and read rh (s) and the
        // diagonal when there is one (2 or 3 N), plus the apply's result: the output vector (N), or with
        // the patch source the patch buffer, the essential flags and the apply's input on the essential
        // rows (counted as the flags: the rows are few)
        const double diag = c->bcgs_diag ? 1.0 : 0.0;
        const double S = kBrick * c->p + 1.0;
        const double src = c->bcgs_src ? 8.0 * S * S * S * (double)c->nblk + 1.0 * nl : 8.0 * nl;
        return 8.0 * nl * (4 + 3 + 7) + 2.0 * (8.0 * nl * (2.0 + diag) + src);
    }
    if (c->fa_ready) {  // CSR SpMV: values + columns + row pointers + x + y
        if (k != CDFEM_K_APPLY) throw ArgError("FA operators report the SpMV (CDFEM_K_APPLY) only");
        // (SELL adds < 1 % padding; 16-bit column deltas when the bandwidth fits)
        // 8 B value + 2 B delta per entry (4 B column in the 32-bit slices of a mixed layout); LDS
        // windows: 8 B value + 2 B window position per entry, 4 B per staged column (the x values
        // themselves: 8 B per row, each window's halo beyond its own rows from L2)
        if (c->lds_rows > 0)
            return 10.0 * (double)c->nnz + 4.0 * (double)c->lds_halo + 4.0 * (double)(c->nslices + 1) +
                   16.0 * nl;
        return spmv_delta(c) ? 10.0 * (double)c->nnz + 2.0 * (double)c->sell_nnz_wide + 4.0 * (nl + 1) + 16.0 * nl +
                                   (c->d_swide ? (double)c->nslices : 0.0)
                             : 12.0 * (double)c->nnz + 4.0 * (nl + 1) + 16.0 * nl;
    }
    const double nq = nq_of(c, c->rule_op);
    if (use_hobrick_cg(c) && (k == CDFEM_K_APPLY || k == CDFEM_K_UPDATE)) {
        // the high-order brick CG: factors + gathered r, M^-1, d + ess flags + d (writer) + patch
        // outputs (+ x read and written under the x-fold); update: r, M^-1, ess, r write + patches
        const double S = brick_patch_side(c), SZ = brick_patch_side_z(c);
        const double patches = 8.0 * S * S * SZ * (double)brick_count(c);
        const bool xf = c->cg_xfold != 0;
        // (ho_uniform: one element matrix in operand order, 16 x 4 padded, instead of the factor stream)
        const double nrow = 16.0 * ((c->nd + 15) / 16), ncol = 4.0 * ((c->nd + 3) / 4);
        const double fac = ho_uniform_elem(c) ? 8.0 * nrow * ncol : 8.0 * c->ncomp * ne;
        return k == CDFEM_K_APPLY ? fac + 33.0 * nl + patches + (xf ? 16.0 * nl : 0.0)
                                  : (xf ? 25.0 : 49.0) * nl + patches;
    }
    if (use_brick(c)) {
        // CG-mode brick kernels (what the Krylov loop launches); see DESIGN.md section 4
        const int64_t s1 = (int64_t)kBrick * c->p;
        int64_t nface_dofs = 0;
        for (int64_t z = 0; z < c->Lz; ++z)
            for (int64_t y = 0; y < c->Ly; ++y) {
                if (z % s1 == 0 || y % s1 == 0) { nface_dofs += c->Lx; continue; }
                nface_dofs += (c->Lx - 1) / s1 + 1;
            }
        const double nf = (double)nface_dofs;
        const double S = kBrick * c->p + 1.0;
        const double patches = 8.0 * S * S * S * (double)c->nblk;  // the CG apply's patch outputs
        // x-fold (cg_xfold, Kronecker form): x += alpha d moves from the update into the apply
        const bool xf = c->cg_xfold != 0 && pa_af(c) == 2;
        switch (k) {
        case CDFEM_K_APPLY:   // qdata (or per-element affine factors) + gathered r, M^-1, d + ess
                              // flags + d (each dof by its one writer brick) + patch outputs
                              // (+ x read and written by its writer brick under the x-fold)
            // (pa_uniform: one element matrix, 14 x 64 operand doubles, instead of the factor stream)
            // (pa_geom: the element's mask and 21 map coefficients instead of its stream)
            // (pa_uniform_diag: the 64-entry class table instead of the gathered M^-1)
            return (uniform_elem(c) ? 8.0 * 14 * 64
                    : pa_geom_on(c) ? 8.0 * GeomLayout::kNC * ne
                                    : 8.0 * c->ncomp * (c->d_qaff ? 1.0 : nq) * ne) +
                   (uniform_diag(c) ? 16.0 * nl + 8.0 * kUdiagN : 24.0 * nl) + 1.0 * nl + 8.0 * nl + patches +
                   (xf ? 16.0 * nl : 0.0);
        case CDFEM_K_E2L:     // the Mult's row sums: the patch buffer + ess flags + y (brick_mult_pb,
                              // Kronecker form), or face partials + x, ess, y of the face dofs
            return (c->brick_mult_pb && pa_af(c) == 2) ? patches + 9.0 * nl
                                                       : 8.0 * c->nface * (double)c->nblk + 25.0 * nf;
        case CDFEM_K_UPDATE:  // x, d, r, M^-1 read, ess, x, r write + the patch outputs (each once);
                              // x-fold: r, M^-1, ess and r write only
            // (pa_uniform_diag: no M^-1 stream; the essential flag it reads instead is counted above)
            return (xf ? 25.0 : 49.0) * nl + patches - (uniform_diag(c) ? 8.0 * nl : 0.0);
        default: throw ArgError("kernel not launched on the brick path");
        }
    }
    // the 3D applies on affine factors read one factor set per element (the 2D apply streams)
    const double nqs = (c->qlay == 1 ? tile_affine(c) : (c->dim == 3 && c->d_qaff != nullptr)) ? 1.0 : nq;
    // (ho_geom: the tile apply reads the element's 24 doubles of map coefficients instead of its stream)
    const bool hgeo = c->qlay == 1 && ho_geom_on(c);
    switch (k) {
    case CDFEM_K_APPLY:
        if (c->epencil)  // lattice gather: x + ess flags (each L-dof once) + qdata + E-vector write
            return 9.0 * nl + (hgeo ? 8.0 * HoGeomLayout::kNC * ne : 8.0 * c->ncomp * nqs * ne) + 8.0 * nd * ne +
                   (tile_dfold_ok(c) ? 16.0 * nl : 0.0);  // CG apply with the direction fold:
                                                          // + d_old gather, + d store
        // x gather (each L-dof once) + qdata stream + element map + E-vector write
        // (pa_geom: the element's mask and 21 map coefficients instead of its stream)
        return 8.0 * nl + (c->qlay == 0 && c->dim == 3 && pa_geom_on(c) ? 8.0 * GeomLayout::kNC * ne
                           : hgeo                                       ? 8.0 * HoGeomLayout::kNC * ne
                                                                        : 8.0 * c->ncomp * nqs * ne) +
               4.0 * nd * ne + 8.0 * nd * ne;
    case CDFEM_K_E2L:
        if (c->epencil)  // E-vector read + ess flags + y write + x read (constraint / dot)
            return 8.0 * nd * ne + 1.0 * nl + 8.0 * nl + 8.0 * nl;
        // E-vector read + positions + offsets + y write + x read (constraint / dot)
        return 8.0 * nd * ne + 4.0 * nd * ne + 4.0 * nl + 8.0 * nl + 8.0 * nl;
    case CDFEM_K_UPDATE: return 8.0 * nl * 8;     // x,d,r,z,dinv read; x,r,z write
    case CDFEM_K_DIRECTION: return 8.0 * nl * 3;  // z,d read; d write
    default: throw ArgError("bad kernel id");
    }
}

}  // namespace cdfem
