// newton.hip — the nonlinear heat form's entry points (include/cdfem.h: cdfem_nl_*, cdfem_bdr_*) and the
// device-resident Newton driver behind cdfem_newton_solve (the reference's NewtonPetscSolver::Solve,
// newton_petsc_solver.hpp:180-259).  Host-side orchestration only: the residual, the Jacobian's element
// matrices and the boundary load are formed by nl_kernels.hip, the sums and the assembly by the kernels of the
// linear paths (k_e2l, k_fa_gather, k_fa_eliminate, k_sell_fill), each linear solve by solve.hip's drivers.
// On quads and hexes (cdfem_nl_pa_setup) the form is matrix-free: nl_tensor.hip's one kernel gives the residual,
// and the Jacobian is a copy of u that the linear operator's launch points hand to the same kernel.  After
// cdfem_nl_fa_setup the residual is the same kernel and the Jacobian is assembled as on simplices, its element
// matrices by nl_fa_tensor.hip.
//
// Host / device traffic of one Newton iteration: the residual norm and the update norm (8 bytes each, after
// a one-block reduction) and whatever the linear solver polls; u, R, dx and u_old never leave the device.
// The three timers synchronise the stream around their sections, so an iteration has three more host waits
// than it needs; they are the reference's timers (result.timing) and are kept for that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "cdfem_internal.hpp"
#include "host_util.hpp"

using namespace cdfem;

namespace {

using Clock = std::chrono::steady_clock;

// the stream idle, then the clock
Clock::time_point tick(cdfem_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    return Clock::now();
}
double since(cdfem_ctx *c, Clock::time_point t0) { return std::chrono::duration<double>(tick(c) - t0).count(); }

// a simplex mesh on one rank, else CDFEM_ERR_UNSUPPORTED
void require_simplex_one_rank(cdfem_ctx *c, const char *what)
{
    require_mesh(c);
    if (multi_rank(c)) throw UnsupportedError(std::string(what) + " runs on one rank");
    if (c->geom != 1) throw UnsupportedError(std::string(what) + " is implemented for simplex meshes");
}

// after cdfem_nl_setup (simplices) or cdfem_nl_pa_setup / cdfem_nl_fa_setup (quads / hexes: heat.tensor, with
// heat.assembled telling the two apart), on one rank
void require_nl(cdfem_ctx *c)
{
    require_mesh(c);
    if (multi_rank(c)) throw UnsupportedError("the nonlinear heat form runs on one rank");
    if (!c->heat.ready || c->heat.tensor != (c->geom == 0))
        throw StateError(c->geom == 0 ? "neither cdfem_nl_pa_setup nor cdfem_nl_fa_setup has been called"
                                      : "cdfem_nl_setup has not been called");
}

// what the two quad / hex setups share (inside guarded): the refusals, the operator of the previous setup
// dropped, the rule
void nl_tensor_setup(cdfem_ctx *c, const cdfem_nl_heat_coeffs *k, const char *what)
{
    require_mesh(c);
    if (multi_rank(c)) throw UnsupportedError("the nonlinear heat form runs on one rank");
    if (c->geom != 0) throw UnsupportedError("simplex meshes take the assembled form: cdfem_nl_setup");
    if (!nl_tensor_supported(c->dim, c->p))
        throw UnsupportedError(std::string(what) + " is built for quads p = 1..3 and hexes p = 1, 2");
    if (!k) throw ArgError("null coefficients");
    if (!(k->dt > 0.0)) throw ArgError("dt must be positive");
    NlState &S = c->heat;
    S.ready = false;
    if (S.jac_mf) {  // (a Jacobian of the previous coefficients is no operator any more)
        S.jac_mf = false;
        c->dinv_ready = false;
    }
    if (c->fa_ready) {  // an assembled operator of this mesh (linear, or a Jacobian) is dropped, as cdfem_pa_setup drops it
        c->fa_ready = false;
        c->dinv_ready = false;
        ilu_free(c);
    }
    // IntRules.Get(geom, 2p + OrderW + 2) with OrderW = dim - 1 on the multilinear map: order 2p + 3 / 2p + 4,
    // which MFEM's tensor Gauss-Legendre rules meet with p + 2 / p + 3 points per direction
    S.rule = make_rule(c->p, nl_tensor_points_1d(c->dim, c->p));
    S.nq = nq_of(c, S.rule);
}

// what both setup calls share: the coefficients, the Newton vectors, u_old = 0 and g = 0, an empty history
void nl_init_state(cdfem_ctx *c, const cdfem_nl_heat_coeffs *k)
{
    NlState &S = c->heat;
    for (DevBuf<double> *v : {&S.d_u, &S.d_R, &S.d_rhs, &S.d_dx, &S.d_uold, &S.d_g}) v->alloc(c->nl);
    S.d_norm.alloc(1);
    HIPCHK(hipMemsetAsync(S.d_uold, 0, c->nl * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(S.d_g, 0, c->nl * sizeof(double), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (the callers' host tables die at scope exit)
    S.dt = k->dt; S.a0 = k->a0; S.a1 = k->a1; S.m0 = k->m0; S.m1 = k->m1; S.u_ref = k->u_ref;
    S.hist_res.clear(); S.hist_upd.clear(); S.hist_lin.clear();
}

// n doubles from src (host or device) into the device buffer dst
void copy_in(cdfem_ctx *c, double *dst, const double *src, int where, size_t n)
{
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double),
                          where == CDFEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
}

// R = residual(u): element vectors, their sums in ascending element order, then - g and the essential rows
// zeroed; negR (may be null) = -R
void nl_residual(cdfem_ctx *c, const double *u, double *R, double *negR)
{
    if (c->heat.tensor)
        timed(c, CDFEM_K_NL_RESIDUAL, [&] { HIPCHK(launch_nl_tensor(c, 0, u, nullptr, false, c->d_Ye, nullptr)); });
    else
        HIPCHK(launch_nl_residual(c, u, c->d_Ye));
    HIPCHK(launch_e2l(c, c->d_Ye, nullptr, R, false, 0));
    HIPCHK(launch_nl_finish(c, R, c->heat.d_g, negR));
}

// J(u) becomes the assembled operator: the element matrices in k_simplex_elem's layout, then the full
// assembly's own gather, elimination and SELL fill; what belonged to the previous operator is dropped
// On quads and hexes after cdfem_nl_pa_setup nothing is assembled: J(u) becomes the current operator as a copy
// of u, which the launch points of the linear operator hand to k_nl_tensor (launch_apply_st, launch_diag_elem);
// after cdfem_nl_fa_setup the element matrices are nl_fa_tensor.hip's and the rest is the simplex sequence
void nl_jacobian(cdfem_ctx *c, const double *u)
{
    if (c->heat.tensor && !c->heat.assembled) {
        NlState &S = c->heat;
        if (u != S.d_ulin.get())
            HIPCHK(hipMemcpyAsync(S.d_ulin, u, c->nl * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->kinds = CDFEM_DIFFUSION | CDFEM_CONVECTION | CDFEM_MASS;
        S.jac_mf = true;
        c->pa_ready = false;  // (the linear operator's point data no longer describe the current operator)
        c->fa_ready = false;
        c->dinv_ready = false;
        ilu_free(c);  // (factors of an assembled linear operator on this mesh)
        return;
    }
    fa_ensure_pattern(c);
    if (c->heat.tensor) {
        timed(c, CDFEM_K_NL_ASSEMBLE, [&] { HIPCHK(launch_nl_tensor_elem(c, u)); });
        timed(c, CDFEM_K_FA_GATHER, [&] { HIPCHK(launch_fa_assemble(c)); });
        timed(c, CDFEM_K_SELL_FILL, [&] { HIPCHK(launch_sell_fill(c)); });
    } else {
        HIPCHK(launch_nl_gradient(c, u));
        HIPCHK(launch_fa_assemble(c));
        HIPCHK(launch_sell_fill(c));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->kinds = CDFEM_DIFFUSION | CDFEM_CONVECTION | CDFEM_MASS;
    c->fa_ready = true;
    c->pa_ready = false;
    c->dinv_ready = false;
    ilu_free(c);  // factors belong to the previous operator
}

// ||v||_2: the deterministic dot's one-block sum, 8 bytes to the host
double norm2(cdfem_ctx *c, const double *v)
{
    double s = 0.0;
    HIPCHK(launch_dot(c, v, v, c->heat.d_norm));
    HIPCHK(hipMemcpyAsync(&s, c->heat.d_norm, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return std::sqrt(s);
}

// points of the boundary rule on the reference facet (dim - 1 coordinates each): Gauss-Legendre on [0, 1]
// with (p + 1) / 2 + 1 points, or MFEM's tabulated triangle rule of order p + 1
int facet_rule(int dim, int p, std::vector<double> &xi, std::vector<double> &w)
{
    if (dim == 2) {
        const int n = (p + 1) / 2 + 1;
        xi.resize(n);
        w.resize(n);
        gauss_legendre(n, xi.data(), w.data());
        return n;
    }
    return simplex_rule_for_order(2, p + 1, xi, w);
}

}  // namespace

extern "C" {

int cdfem_nl_setup(cdfem_ctx *c, const cdfem_nl_heat_coeffs *k)
{
    return guarded(c, [&] {
        require_simplex_one_rank(c, "the nonlinear heat form");
        if (!k) throw ArgError("null coefficients");
        if (!(k->dt > 0.0)) throw ArgError("dt must be positive");
        NlState &S = c->heat;
        S.ready = false;
        const int dim = c->dim, nd = c->nd, p = c->p;
        // the one rule of both integrators, order 2p + 2; tables in d_stab's layout, from the 1-ulp basis (u and
        // grad u are interpolated from nodal values: simplex_basis_x says what a table error would cost)
        std::vector<double> w;
        S.nq = simplex_rule_for_order(dim, 2 * p + 2, S.h_sxi, w);
        const int nq = S.nq;
        std::vector<double> tab((size_t)nq * nd * (dim + 1) + nq);
        for (int q = 0; q < nq; ++q) {
            double phi[10], dphi[30];
            simplex_basis_x(dim, p, &S.h_sxi[(size_t)q * dim], phi, dphi);
            for (int i = 0; i < nd; ++i) {
                tab[(size_t)q * nd + i] = phi[i];
                for (int a = 0; a < dim; ++a) tab[(size_t)nq * nd + ((size_t)q * nd + i) * dim + a] = dphi[i * dim + a];
            }
            tab[(size_t)nq * nd * (dim + 1) + q] = w[q];
        }
        upload(c, S.d_tab, tab);
        upload(c, S.d_edofs, c->h_dofs);
        nl_init_state(c, k);
        S.tensor = false;
        S.assembled = false;
        S.ready = true;
        return CDFEM_OK;
    });
}

int cdfem_nl_pa_setup(cdfem_ctx *c, const cdfem_nl_heat_coeffs *k)
{
    return guarded(c, [&] {
        nl_tensor_setup(c, k, "the matrix-free nonlinear form");
        NlState &S = c->heat;
        S.d_ulin.alloc(c->nl);
        nl_init_state(c, k);
        S.tensor = true;
        S.assembled = false;
        S.ready = true;
        return CDFEM_OK;
    });
}

int cdfem_nl_fa_setup(cdfem_ctx *c, const cdfem_nl_heat_coeffs *k)
{
    return guarded(c, [&] {
        nl_tensor_setup(c, k, "the assembled tensor Jacobian");
        NlState &S = c->heat;
        fa_ensure_pattern(c);  // (may refuse: before any state of this setup exists)
        upload(c, S.d_edofs, c->h_dofs);
        S.d_jq.alloc(nl_fa_tensor_state_size(c));
        nl_init_state(c, k);
        S.tensor = true;
        S.assembled = true;
        S.ready = true;
        return CDFEM_OK;
    });
}

int cdfem_nl_set_old(cdfem_ctx *c, const double *u_old, int where)
{
    return guarded(c, [&] {
        require_nl(c);
        if (!u_old) throw ArgError("null vector");
        copy_in(c, c->heat.d_uold, u_old, where, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->heat.jac_mf) c->dinv_ready = false;  // the matrix-free J reads the current u_old
        return CDFEM_OK;
    });
}

int cdfem_nl_set_rhs(cdfem_ctx *c, const double *g, int where)
{
    return guarded(c, [&] {
        require_nl(c);
        if (g) copy_in(c, c->heat.d_g, g, where, c->nl);
        else HIPCHK(hipMemsetAsync(c->heat.d_g, 0, c->nl * sizeof(double), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

int cdfem_nl_residual(cdfem_ctx *c, const double *u, double *R, int where)
{
    return guarded(c, [&] {
        require_nl(c);
        if (!u || !R) throw ArgError("null vector");
        const double *du = dev_in(c, u, where, c->heat.d_u, c->nl);
        double *dR = where == CDFEM_DEVICE ? R : c->heat.d_R.get();
        nl_residual(c, du, dR, nullptr);
        dev_out(c, R, where, dR, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        prof_collect(c);
        return CDFEM_OK;
    });
}

int cdfem_nl_gradient(cdfem_ctx *c, const double *u, int where)
{
    return guarded(c, [&] {
        require_nl(c);
        if (!u) throw ArgError("null vector");
        nl_jacobian(c, dev_in(c, u, where, c->heat.d_u, c->nl));
        prof_collect(c);
        return CDFEM_OK;
    });
}

int cdfem_newton_solve(cdfem_ctx *c, const cdfem_newton_params *prm, const cdfem_solver_params *lin, double *u,
                       int where, cdfem_newton_result *res)
{
    return guarded(c, [&] {
        require_nl(c);
        if (!prm || !lin || !u || !res) throw ArgError("null argument");
        *res = cdfem_newton_result{};
        check_solver_params(*lin);
        // the reference's defaults (NewtonConfig)
        const double abs_tol = prm->abs_tol > 0.0 ? prm->abs_tol : 1e-10;
        const double rel_tol = prm->rel_tol > 0.0 ? prm->rel_tol : 1e-8;
        const int max_iter = prm->max_iter > 0 ? prm->max_iter : 20;
        const int freq = std::max(1, prm->jacobian_rebuild_freq);
        NlState &S = c->heat;
        S.hist_res.clear(); S.hist_upd.clear(); S.hist_lin.clear();
        const auto record = [&](double rn, double un, int its) {
            S.hist_res.push_back(rn);
            S.hist_upd.push_back(un);
            S.hist_lin.push_back(its);
        };
        copy_in(c, S.d_u, u, where, c->nl);
        double r0 = 1.0, du0 = 1.0;
        bool have_jacobian = false;
        for (int iter = 0; iter < max_iter; ++iter) {
            auto t0 = tick(c);
            nl_residual(c, S.d_u, S.d_R, S.d_rhs);
            const double rn = norm2(c, S.d_R);
            res->residual_seconds += since(c, t0);
            if (iter == 0) {
                r0 = std::max(1.0, rn);
                res->initial_residual = r0;
            }
            const double rel = rn / r0;
            res->final_residual = rn;
            res->final_relative_residual = rel;
            if (rn < abs_tol || rel < rel_tol) {
                res->converged = 1;
                res->iterations = iter;
                record(rn, 0.0, 0);
                if (prm->print_level > 0) std::printf("newton %3d  |R| %.6e  rel %.6e  converged\n", iter, rn, rel);
                break;
            }
            if (iter % freq == 0 || !have_jacobian) {
                t0 = tick(c);
                nl_jacobian(c, S.d_u);
                have_jacobian = true;
                res->jacobian_seconds += since(c, t0);
            }
            t0 = tick(c);
            cdfem_solver_result lr{};
            c->last_method = lin->method;
            solve_mesh_order(c, *lin, S.d_rhs, S.d_dx, lr);  // zero initial guess, B and X on the device
            res->linear_seconds += since(c, t0);
            res->linear_iterations += lr.iterations;
            if (!lr.converged) {  // (the reference throws)
                record(rn, 0.0, lr.iterations);
                res->iterations = iter;
                dev_out(c, u, where, S.d_u, c->nl);
                HIPCHK(hipStreamSynchronize(c->stream));
                const std::string inner = c->err.empty() ? std::string() : " (" + c->err + ")";
                c->err = "Newton iteration " + std::to_string(iter) + ": the linear solve did not converge in " +
                         std::to_string(lr.iterations) + " iterations, residual " + std::to_string(lr.final_norm) + inner;
                return (int)CDFEM_ERR_NOT_CONVERGED;
            }
            const double un = norm2(c, S.d_dx);
            if (iter == 0) {
                du0 = std::max(1.0, un);
                res->initial_update_norm = du0;
            }
            res->final_update_norm = un;
            HIPCHK(launch_axpby(c, 1.0, S.d_dx, 1.0, S.d_u));  // essential entries: dx = 0 there
            record(rn, un, lr.iterations);
            if (prm->print_level > 0)
                std::printf("newton %3d  |R| %.6e  rel %.6e  |dx| %.6e  linear its %d\n", iter, rn, rel, un, lr.iterations);
        }
        if (!res->converged) res->iterations = max_iter;
        dev_out(c, u, where, S.d_u, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!res->converged) {
            c->err = "Newton: no convergence in " + std::to_string(max_iter) + " iterations";
            return (int)CDFEM_ERR_NOT_CONVERGED;
        }
        return (int)CDFEM_OK;
    });
}

int cdfem_newton_history(cdfem_ctx *c, double *res, double *upd, int32_t *lin_its, int cap, int *count)
{
    return guarded(c, [&] {
        const NlState &S = c->heat;
        const int n = (int)S.hist_res.size();
        if (count) *count = n;
        for (int i = 0; i < std::min(cap, n); ++i) {
            if (res) res[i] = S.hist_res[i];
            if (upd) upd[i] = S.hist_upd[i];
            if (lin_its) lin_its[i] = S.hist_lin[i];
        }
        return CDFEM_OK;
    });
}

int cdfem_bdr_set(cdfem_ctx *c, int nbf, const int32_t *face_elem, const int32_t *face_local)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (multi_rank(c)) throw UnsupportedError("the boundary linear form runs on one rank");
        const bool tensor = c->geom == 0;
        if (tensor && !nl_tensor_supported(c->dim, c->p))
            throw UnsupportedError("the boundary linear form on quad / hex faces is built for quads p = 1..3 and hexes p = 1, 2");
        if (nbf < 0 || (nbf > 0 && (!face_elem || !face_local))) throw ArgError("bad facet list");
        const int dim = c->dim, p = c->p, nd = c->nd, d1 = p + 1;
        const int nfd = tensor ? (dim == 3 ? d1 * d1 : d1) : facet_ndofs(dim, p);
        const int nfl = tensor ? 2 * dim : dim + 1;  // local facets of an element
        if ((int64_t)nbf * nfd >= ((int64_t)1 << 31)) throw ArgError("facet E-vector exceeds int32 indexing");
        for (int t = 0; t < nbf; ++t) {
            if (face_elem[t] < 0 || face_elem[t] >= c->ne) throw ArgError("facet element out of range");
            if (face_local[t] < 0 || face_local[t] >= nfl) throw ArgError("local facet out of range");
        }
        NlState &S = c->heat;
        S.nbf = 0;
        S.d_b_off.reset();
        std::vector<double> xi, w, bxi, btab, bverts;
        int nqb = 0, nqb1 = 0;
        // quad / hex facet f = 2 axis + side: the axes that remain, ascending
        const auto rem = [&](int axis, int s) { return s == 0 ? (axis == 0 ? 1 : 0) : (axis == 2 ? 1 : 2); };
        if (tensor) {
            // BoundaryLFIntegrator's order p + 1 on segments and squares: MFEM's tensor Gauss-Legendre rule with
            // (p + 1) / 2 + 1 points per direction, the lower remaining axis fastest
            nqb1 = (p + 1) / 2 + 1;
            nqb = dim == 3 ? nqb1 * nqb1 : nqb1;
            const Rule1D r = make_rule(p, nqb1);
            btab.resize((size_t)nqb1 * (d1 + 2));
            for (int q = 0; q < nqb1; ++q) {
                for (int d = 0; d < d1; ++d) btab[(size_t)q * d1 + d] = r.B[q][d];
                btab[(size_t)nqb1 * d1 + q] = r.pts[q];
                btab[(size_t)nqb1 * (d1 + 1) + q] = r.wts[q];
            }
            bxi.resize((size_t)nfl * nqb * dim);
            for (int f = 0; f < nfl; ++f)
                for (int q = 0; q < nqb; ++q) {
                    double *x = &bxi[((size_t)f * nqb + q) * dim];
                    x[f >> 1] = f & 1;
                    x[rem(f >> 1, 0)] = r.pts[q % nqb1];
                    if (dim == 3) x[rem(f >> 1, 1)] = r.pts[q / nqb1];
                }
            // the facets' element vertices (quads and hexes keep their geometry on the device alone)
            const size_t nvd = (size_t)c->nv * dim;
            std::vector<double> verts((size_t)c->ne * nvd);
            HIPCHK(hipMemcpy(verts.data(), c->d_verts, verts.size() * sizeof(double), hipMemcpyDeviceToHost));
            bverts.resize((size_t)nbf * nvd);
            for (int t = 0; t < nbf; ++t)
                std::copy_n(&verts[(size_t)face_elem[t] * nvd], nvd, &bverts[(size_t)t * nvd]);
        } else {
            nqb = facet_rule(dim, p, xi, w);
            bxi.resize((size_t)(dim + 1) * nqb * dim);
            btab.resize((size_t)(dim + 1) * nqb * nfd + nqb);
        }
        // simplices: facet f's points in the element's reference coordinates (vertex 0 at the origin, vertex k at
        // e_k; the facet's vertices ascending), and the facet dofs' basis values there
        for (int f = 0; !tensor && f <= dim; ++f) {
            int v[3], m = 0;
            for (int a = 0; a <= dim; ++a)
                if (a != f) v[m++] = a;
            for (int q = 0; q < nqb; ++q) {
                double *x = &bxi[((size_t)f * nqb + q) * dim];
                for (int k = 0; k < dim; ++k) {
                    const auto V = [&](int a) { return a == k + 1 ? 1.0 : 0.0; };  // coordinate k of vertex a
                    x[k] = V(v[0]);
                    for (int s = 1; s < dim; ++s) x[k] += xi[(size_t)q * (dim - 1) + s - 1] * (V(v[s]) - V(v[0]));
                }
                double phi[10], dphi[30];
                simplex_basis_x(dim, p, x, phi, dphi);
                for (int l = 0; l < nfd; ++l) btab[((size_t)f * nqb + q) * nfd + l] = phi[facet_dof(dim, p, f, l)];
            }
        }
        for (int q = 0; !tensor && q < nqb; ++q) btab[(size_t)(dim + 1) * nqb * nfd + q] = w[q];
        // per dof its entries of the facet E-vector [nbf][nfd], ascending facet
        std::vector<int32_t> off(c->nl + 1, 0), pos((size_t)nbf * nfd);
        const auto gdof = [&](int t, int l) {
            const int f = face_local[t];
            if (!tensor) return c->h_dofs[(size_t)face_elem[t] * nd + facet_dof(dim, p, f, l)];
            // the element's lexicographic dofs with axis index 0 or p, the lower remaining axis fastest
            int idx[3] = {0, 0, 0};
            idx[f >> 1] = (f & 1) * p;
            idx[rem(f >> 1, 0)] = l % d1;
            if (dim == 3) idx[rem(f >> 1, 1)] = l / d1;
            return c->h_dofs[(size_t)face_elem[t] * nd + idx[0] + d1 * (idx[1] + d1 * idx[2])];
        };
        for (int t = 0; t < nbf; ++t)
            for (int l = 0; l < nfd; ++l) off[gdof(t, l) + 1]++;
        for (int64_t i = 0; i < c->nl; ++i) off[i + 1] += off[i];
        {
            std::vector<int32_t> fill(off.begin(), off.end() - 1);
            for (int t = 0; t < nbf; ++t)
                for (int l = 0; l < nfd; ++l) pos[fill[gdof(t, l)]++] = t * nfd + l;
        }
        S.h_face_elem.assign(face_elem, face_elem + nbf);
        S.h_face_local.assign(face_local, face_local + nbf);
        S.h_bxi = bxi;
        S.h_bverts = bverts;
        upload(c, S.d_face_elem, S.h_face_elem);
        upload(c, S.d_face_local, S.h_face_local);
        upload(c, S.d_btab, btab);
        upload(c, S.d_b_pos, pos);
        S.d_bYe.alloc(std::max<size_t>(1, (size_t)nbf * nfd));
        S.d_bgq.alloc(std::max<size_t>(1, (size_t)nbf * nqb));
        upload(c, S.d_b_off, off);
        HIPCHK(hipStreamSynchronize(c->stream));  // the host tables die at scope exit
        S.nqb = nqb;
        S.nqb1 = nqb1;
        S.nfd = nfd;
        S.nbf = nbf;
        return CDFEM_OK;
    });
}

static void require_bdr(cdfem_ctx *c)
{
    require_mesh(c);
    if (!c->heat.d_b_off) throw StateError("cdfem_bdr_set has not been called");
}

int cdfem_bdr_rule_size(cdfem_ctx *c, int *nq)
{
    return guarded(c, [&] {
        require_bdr(c);
        if (!nq) throw ArgError("nq is null");
        *nq = c->heat.nqb;
        return CDFEM_OK;
    });
}

int cdfem_bdr_quadrature_points(cdfem_ctx *c, double *xyz, int where)
{
    return guarded(c, [&] {
        require_bdr(c);
        if (!xyz) throw ArgError("xyz is null");
        const NlState &S = c->heat;
        const int dim = c->dim, nv = dim + 1, nqb = S.nqb;
        std::vector<double> out((size_t)S.nbf * nqb * dim);
        for (int t = 0; c->geom == 0 && t < S.nbf; ++t) {  // quads / hexes: the multilinear map, on the host
            const double *V = &S.h_bverts[(size_t)t * c->nv * dim];
            const double *X = &S.h_bxi[(size_t)S.h_face_local[t] * nqb * dim];
            for (int q = 0; q < nqb; ++q)
                for (int k = 0; k < dim; ++k) {
                    double x = 0.0;
                    for (int v = 0; v < c->nv; ++v) {
                        double N = 1.0;
                        for (int m = 0; m < dim; ++m) N *= ((v >> m) & 1) ? X[(size_t)q * dim + m] : 1.0 - X[(size_t)q * dim + m];
                        x += N * V[v * dim + k];
                    }
                    out[((size_t)t * nqb + q) * dim + k] = x;
                }
        }
        for (int t = 0; c->geom != 0 && t < S.nbf; ++t) {  // affine simplices: x = v0 + J xi, evaluated on the host
            const double *V = &c->h_verts[(size_t)S.h_face_elem[t] * nv * dim];
            const double *X = &S.h_bxi[(size_t)S.h_face_local[t] * nqb * dim];
            for (int q = 0; q < nqb; ++q)
                for (int k = 0; k < dim; ++k) {
                    double x = V[k];
                    for (int m = 0; m < dim; ++m) x += (V[(m + 1) * dim + k] - V[k]) * X[(size_t)q * dim + m];
                    out[((size_t)t * nqb + q) * dim + k] = x;
                }
        }
        if (where == CDFEM_DEVICE) {
            HIPCHK(hipMemcpyAsync(xyz, out.data(), out.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        } else {
            std::copy(out.begin(), out.end(), xyz);
        }
        return CDFEM_OK;
    });
}

int cdfem_bdr_lf_assemble(cdfem_ctx *c, const double *g_q, double *b, int where)
{
    return guarded(c, [&] {
        require_bdr(c);
        if (!b || (c->heat.nbf > 0 && !g_q)) throw ArgError("null vector");
        NlState &S = c->heat;
        if (S.nbf > 0) copy_in(c, S.d_bgq, g_q, where, (size_t)S.nbf * S.nqb);
        double *db = where == CDFEM_DEVICE ? b : c->d_w[1].get();
        HIPCHK(launch_bdr_lf(c, S.d_bgq, db));
        dev_out(c, b, where, db, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

}  // extern "C"
