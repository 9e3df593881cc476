/*
 * cdfem.h — C-ABI of the MI355X-native convection-diffusion FE hot path (libcdfem.so).
 *
 * One opaque context per GPU (per process / rank).  All entry points return CDFEM_OK (0) or an
 * error code; the message is in cdfem_last_error(ctx).  No C++ exception crosses this boundary;
 * the C++ MFEM-shaped layer (continuum-mechanics-mfem_amd/cpp/cdfem_mfem.hpp) turns a status into
 * std::runtime_error, which the reference drivers already map to exit code 3
 * (linear_convection_diffusion_2D.cpp:435-442).
 *
 * Each entry point names the reference interface it replaces.  The reference calls MFEM, hypre
 * and PETSc (not vendored: SURVEY.md §8b/c), so the "replaces" lines cite the reference CALL SITE.
 *
 * Ownership: the caller owns every host array; the context owns every device buffer it allocates;
 * no caller pointer is retained after a call returns.  Pointers tagged `where` are host memory
 * when where == CDFEM_HOST and device memory (hipMalloc / cdfem_alloc) when where == CDFEM_DEVICE.
 * A context is not thread-safe.  Calls with where == CDFEM_HOST are synchronous on return.
 *
 * Vector spaces.  L-vector = all dofs of the rank's elements (for one rank this is also MFEM's
 * T-vector: P = I on a conforming mesh).  DoF numbering and element-dof maps are supplied by the
 * caller; element dofs are LEXICOGRAPHIC on the tensor element (l = dx + (p+1)(dy + (p+1)dz)),
 * element vertices lexicographic (v = a + 2b + 4c), reference element [0,1]^dim.
 */
#ifndef CDFEM_H
#define CDFEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDFEM_ABI_VERSION 1

typedef struct cdfem_ctx cdfem_ctx;

enum cdfem_status {
    CDFEM_OK = 0,
    CDFEM_ERR_ARG = 1,          /* bad argument / shape mismatch                          */
    CDFEM_ERR_HIP = 2,          /* HIP runtime error (no device, OOM, launch failure)     */
    CDFEM_ERR_STATE = 3,        /* call order violated (e.g. mult before setup)          */
    CDFEM_ERR_UNSUPPORTED = 4,  /* dim/order/kernel combination not built                 */
    CDFEM_ERR_NOT_CONVERGED = 5,/* Krylov solve hit max_iter (result still returned)      */
    CDFEM_ERR_COMM = 6          /* RCCL error                                             */
};

/* integrator kinds (bit mask) */
enum { CDFEM_DIFFUSION = 1, CDFEM_CONVECTION = 2, CDFEM_MASS = 4 };
/* pointer locations */
enum { CDFEM_HOST = 0, CDFEM_DEVICE = 1 };
/* Krylov methods and preconditioners */
enum { CDFEM_CG = 0, CDFEM_GMRES = 1, CDFEM_BICGSTAB = 2 };
enum { CDFEM_PC_NONE = 0, CDFEM_PC_JACOBI = 1, CDFEM_PC_ILU = 2 };
/* quadrature rules whose points the host may need for coefficient evaluation.  Quads / hexes: one
 * operator rule (Gauss n = p + 2, shared by the three integrators; DIFFUSION / CONVECTION / MASS
 * name it too).  Simplices: each integrator its own rule, MFEM's GetRule on affine simplices on
 * MFEM's tabulated rules: DIFFUSION order 2p - 2, CONVECTION and MASS order 2p (OPERATOR refused). */
enum { CDFEM_RULE_OPERATOR = 0, CDFEM_RULE_LINEARFORM = 1, CDFEM_RULE_ERROR = 2, CDFEM_RULE_DIFFUSION = 3,
       CDFEM_RULE_CONVECTION = 4, CDFEM_RULE_MASS = 5,
       CDFEM_RULE_NONLINEAR = 6 /* after cdfem_nl_setup / cdfem_nl_pa_setup / cdfem_nl_fa_setup: the heat form's */ };
/* kernel ids for cdfem_profile_read */
enum { CDFEM_K_APPLY = 0, CDFEM_K_E2L = 1, CDFEM_K_UPDATE = 2, CDFEM_K_DIRECTION = 3, CDFEM_K_ORTH = 4,
       CDFEM_K_NL_RESIDUAL = 5, CDFEM_K_DIAGONAL = 6, /* profiling slots: cdfem_nl_pa_setup's residual kernel;
                                                          the element part of cdfem_pa_diagonal */
       /* one Jacobian rebuild after cdfem_nl_fa_setup, in its three parts: the element matrices (point state and
        * rows), the gather with the elimination, the SELL fill */
       CDFEM_K_NL_ASSEMBLE = 7, CDFEM_K_FA_GATHER = 8, CDFEM_K_SELL_FILL = 9,
       CDFEM_K_COUNT = 10 };

int cdfem_abi_version(void);

/* ---- context ------------------------------------------------------------------------------- */
/* replaces: Device device("cpu") (linear_convection_diffusion_2D.cpp:287) — here: one MI355X.  */
int cdfem_create(int device, cdfem_ctx **out);
void cdfem_destroy(cdfem_ctx *ctx);
const char *cdfem_last_error(const cdfem_ctx *ctx);
int cdfem_synchronize(cdfem_ctx *ctx);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int cdfem_device_count(void);

/* ---- device memory helpers (for where == CDFEM_DEVICE callers and benchmarks) ---------------- */
int cdfem_alloc(cdfem_ctx *ctx, size_t bytes, void **dptr);
int cdfem_free(cdfem_ctx *ctx, void *dptr);
int cdfem_memcpy(cdfem_ctx *ctx, void *dst, int dst_where, const void *src, int src_where, size_t bytes);
/* y = a x + b y on n doubles of device memory, synchronous.  replaces: Vector::Add(a, x) on device
 * vectors (MFEM's forall kernel; diffusion_mms.cpp:433 rhs.Add(dt, f), linear_convection_diffusion_1D.cpp
 * the same rhs update), so the shim's time loop keeps rhs in HBM.                                  */
int cdfem_vec_axpby(cdfem_ctx *ctx, int64_t n, double a, const double *x, double b, double *y);

/* ---- mesh + H1 space -------------------------------------------------------------------------
 * replaces: ParMesh + H1_FECollection(order, dim) + ParFiniteElementSpace + GetEssentialTrueDofs
 *           (linear_convection_diffusion_2D.cpp:300-322; diffusion_mms.cpp:275-285).
 * elem_verts: ne * 2^dim * dim doubles (multilinear geometry), elem_dofs: ne * (order+1)^dim
 * L-dof indices in [0, nldofs), ess_dofs: essential L-dofs (Dirichlet on the marked boundary).  */
int cdfem_mesh_upload(cdfem_ctx *ctx, int dim, int order, int ne, const double *elem_verts,
                      int64_t nldofs, const int32_t *elem_dofs, int n_ess, const int32_t *ess_dofs);

/* Declare the uploaded mesh a structured nx*ny*nz box with the lexicographic numbering of
 * cdfem_box_mesh (validated; element vertices may be perturbed).  Enables the brick fast path:
 * 4x4x4-element bricks per wavefront, E->L sum fused into the apply through LDS, CG direction
 * update fused into the operator gather.  Same results as the generic path to rounding.
 * Call before cdfem_pa_setup.  (Specialisation of ParFiniteElementSpace for Cartesian meshes.)  */
int cdfem_mesh_set_structured(cdfem_ctx *ctx, int nx, int ny, int nz);

/* Physical coordinates of the quadrature points of a rule (CDFEM_RULE_*), ne * nq * dim doubles,
 * element-major, q lexicographic (qx fastest): where a host Coefficient::Eval is sampled
 * (linear_convection_diffusion_2D.cpp:165-215).  cdfem_rule_size returns nq per element.       */
int cdfem_rule_size(cdfem_ctx *ctx, int rule, int *nq_per_elem);
int cdfem_quadrature_points(cdfem_ctx *ctx, int rule, double *xyz, int where);

/* ---- partial assembly (the hot operator) -----------------------------------------------------
 * replaces: a.AddDomainIntegrator(new DiffusionIntegrator(kappa))          :336
 *           a.AddDomainIntegrator(new ConvectionIntegrator(c, alpha))      :337
 *           a.AddDomainIntegrator(new MassIntegrator(s))                   :338
 *           a.Assemble()                                                   :339
 * with MFEM partial-assembly semantics: per-quadrature-point data
 *   D = W kappa adj(J) adj(J)^T / det J,  C = W alpha adj(J) c,  M = W s det J.
 * *_q arrays (ne*nq of the OPERATOR rule = the DIFFUSION / CONVECTION / MASS rules on quads and hexes;
 * conv_q ne*nq*dim) override the constants when
 * non-NULL (host pointers): a variable Coefficient / VectorCoefficient sampled on the host.     */
int cdfem_pa_setup(cdfem_ctx *ctx, unsigned kinds, double kappa, const double *kappa_q,
                   double alpha, const double *conv, const double *conv_q, double mass,
                   const double *mass_q);

/* The same setup with every coefficient form in one struct, including a MatrixCoefficient for the
 * diffusion: DiffusionIntegrator(MatrixCoefficient&) (diffusion_mms_ale.cpp:474-496,1019), the ALE
 * metric alpha dt / J cof(A) cof(A)^T.  The diffusion tensor at a point is K = k I + K_q with k =
 * kappa_q[i] (or kappa) and K_q the symmetric tensor kappa_mat_q[i] (NULL: 0), stored as
 * xx, xy, yy (2D) / xx, xy, xz, yy, yz, zz (3D); qdata D = W adj(J) K adj(J)^T / det J keeps its
 * dim(dim+1)/2 components.  Non-symmetric matrix coefficients are not accepted (the shim checks).  */
typedef struct {
    unsigned kinds;
    double kappa;
    const double *kappa_q;      /* ne*nq, or NULL */
    const double *kappa_mat_q;  /* ne*nq*dim(dim+1)/2, or NULL */
    double alpha;
    const double *conv;         /* 3 doubles (unused components 0) */
    const double *conv_q;       /* ne*nq*dim, or NULL */
    double mass;
    const double *mass_q;       /* ne*nq, or NULL */
} cdfem_form_coeffs;
int cdfem_pa_setup_form(cdfem_ctx *ctx, const cdfem_form_coeffs *form);

/* ---- full assembly: simplex meshes (BASELINE config C4: unstructured tetrahedra), quads and hexes ----
 * replaces: the same ParMesh / H1_FECollection(p, dim) / ParFiniteElementSpace calls on a triangle
 * or tetrahedral mesh (gmsh input, Input/input_2d.yaml:1), and ParBilinearForm::Assemble +
 * FormLinearSystem -> HypreParMatrix (linear_convection_diffusion_2D.cpp:339,349-351) whose CSR
 * PETSc's KSPGMRES then multiplies (MATAIJ, :364-375).
 * cdfem_mesh_upload_simplex: Lagrange P1/P2 (triangles also P3) on affine simplices; elem_verts
 * ne*(dim+1)*dim, elem_dofs ne*nd with nd = dim+1 (P1) / (dim+1)(dim+2)/2 (P2) / 10 (P3 triangle),
 * local order: vertices, then edge nodes along a->b for edges (0,1),(0,2),(0,3),(1,2),(1,3),(2,3)
 * [2D: (0,1),(0,2),(1,2)], then the P3 centroid; det J > 0 required.  cdfem_lf_assemble works on
 * simplex meshes with f sampled at the CDFEM_RULE_LINEARFORM points (MFEM's tabulated rule of order
 * 2p, cdfem_simplex_rule_order).  Each integrator has MFEM's rule (GetRule on affine simplices):
 * diffusion order 2p - 2, convection and mass order 2p, on MFEM's tabulated rules.
 * cdfem_fa_setup: same coefficients as cdfem_pa_setup, per-point arrays on the rule of their
 * integrator: kappa_q / kappa_mat_q on CDFEM_RULE_DIFFUSION, conv_q on CDFEM_RULE_CONVECTION,
 * mass_q on CDFEM_RULE_MASS (cdfem_rule_size / cdfem_quadrature_points);
 * assembles A (CSR, columns sorted) and the eliminated matrix of FormLinearSystem on the GPU.
 * Afterwards cdfem_pa_mult / cdfem_pa_diagonal / cdfem_form_linear_system / cdfem_solve run on the
 * CSR operator.  cdfem_fa_csr exports it (rowptr n+1, cols/vals nnz; pass NULLs to query nnz).
 * Quad and hex meshes (cdfem_mesh_upload): cdfem_fa_setup assembles the same CSR operator, MFEM's default
 * Assemble() (full assembly, :339), on quads of order 1..4 and hexes of order 1, 2, on one rank (other orders
 * and a communicator of several ranks: CDFEM_ERR_UNSUPPORTED).  The three integrators share the one
 * CDFEM_RULE_OPERATOR rule there (Gauss-Legendre, p + 1 points per direction on quads, p + 2 on hexes), and
 * every per-point array (kappa_q, kappa_mat_q, conv_q, mass_q) is sampled at its points, in the order
 * cdfem_quadrature_points(CDFEM_RULE_OPERATOR) returns, as for cdfem_pa_setup.  The assembled operator replaces
 * a partial-assembly one on the same context and the other way round (a later cdfem_pa_setup,
 * cdfem_nl_pa_setup or cdfem_nl_fa_setup drops it, with its Jacobi scale and ILU(0) factors; the pattern is kept
 * for the next cdfem_fa_setup).  On a context declared structured the solves then run the SpMV, not the brick
 * kernels, and CDFEM_PC_ILU becomes available to GMRES and BiCGStab as on simplices.                      */
int cdfem_mesh_upload_simplex(cdfem_ctx *ctx, int dim, int order, int ne, const double *elem_verts,
                              int64_t nldofs, const int32_t *elem_dofs, int n_ess, const int32_t *ess_dofs);
int cdfem_fa_setup(cdfem_ctx *ctx, unsigned kinds, double kappa, const double *kappa_q, double alpha,
                   const double *conv, const double *conv_q, double mass, const double *mass_q);
int cdfem_fa_setup_form(cdfem_ctx *ctx, const cdfem_form_coeffs *form);
int cdfem_fa_csr(cdfem_ctx *ctx, int constrained, int64_t *nnz, int32_t *rowptr, int32_t *cols, double *vals);

/* replaces: Operator::Mult on the assembled operator when constrained == 0 (shared dofs summed over
 * the ranks: P^T A P on a consistent L-vector), the ConstrainedOperator built by FormLinearSystem
 * (:349-351) when constrained == 1 (input essential entries treated as 0, output y[ess] = x[ess]),
 * and BilinearForm::Mult on a ParBilinearForm (diffusion_mms.cpp:430) when constrained == 2: the
 * rank-local product, a partial L-vector (no exchange; the same as 0 on one rank).             */
int cdfem_pa_mult(cdfem_ctx *ctx, const double *x, double *y, int constrained, int where);

/* replaces: BilinearForm::AssembleDiagonal (PA) — unconstrained operator diagonal.             */
int cdfem_pa_diagonal(cdfem_ctx *ctx, double *diag, int where);

/* ---- linear form -----------------------------------------------------------------------------
 * replaces: b.AddDomainIntegrator(new DomainLFIntegrator(f)); b.Assemble()  (:341-343).
 * f_q: values of f at the CDFEM_RULE_LINEARFORM points (ne * nq, host), output b is an L-vector. */
int cdfem_lf_assemble(cdfem_ctx *ctx, const double *f_q, double *b, int where);

/* ---- constrained linear system -----------------------------------------------------------------
 * replaces: a.FormLinearSystem(ess_tdof_list, x, b, A, X, B)  (:349-351), PA/ConstrainedOperator
 * semantics: X = x,  B = b - A x_e (x_e = x on ess dofs, 0 elsewhere),  B[ess] = x[ess].        */
int cdfem_form_linear_system(cdfem_ctx *ctx, const double *x, const double *b, double *X,
                             double *B, int where);

/* ---- Krylov solve ------------------------------------------------------------------------------
 * replaces: PetscLinearSolver(A).Mult(B, X) (:364-375; Input/petsc.opts: gmres, rtol 1e-10,
 * atol 1e-12, max_it 500, pc jacobi) and CGSolver (mesh_recession_handler.cpp:270-276).
 * CG follows MFEM CGSolver (convergence (r,z) <= max(nom0 rel^2, abs^2)); GMRES follows PETSc
 * KSPGMRES (left PC, classical Gram-Schmidt, restart, ||M^{-1} r|| <= max(rtol ||M^{-1}b||, atol)).
 * X on input is ignored (zero initial guess, iterative_mode = false), on output the solution.
 * GMRES: restart 1..64; iterations = inner steps; final_norm = last preconditioned residual
 * estimate (PETSc rnorm).  CDFEM_PC_ILU = ILU(0), natural ordering, no shift: PETSc
 * "-pc_type bjacobi -sub_pc_type ilu" on one rank (Input/petsc_circle.opts:6-8); GMRES on assembled
 * (cdfem_fa_setup) operators, single rank.  Multi-rank slabs: CG and GMRES with none / Jacobi.
 * BiCGStab (CDFEM_BICGSTAB) follows PETSc KSPBCGS with left preconditioning (none, Jacobi, or ILU(0)
 * under GMRES's conditions) and a zero initial guess; restart is ignored.  With r = rh = M^{-1} B,
 * res0 = ||r||, ttol = max(rtol res0, atol), rho_old = alpha = omega_old = 1, p = v = 0, iteration i is
 *   rho = (r, rh); beta = (rho / rho_old)(alpha / omega_old); p = r + beta (p - omega_old v);
 *   v = M^{-1} A p; alpha = rho / (v, rh); s = r - alpha v; t = M^{-1} A s; omega = (s, t) / (t, t);
 *   x += alpha p + omega s; r = s - omega t; converged when ||r|| <= ttol
 * (t = 0: x += alpha p, converged if s = 0).  iterations = these iterations, two operator applies
 * each; initial_norm = res0; final_norm = the last ||r||.  rho = 0, (v, rh) = 0 or t = 0 with s != 0 is
 * a breakdown (PETSc KSP_DIVERGED_BREAKDOWN): CDFEM_ERR_NOT_CONVERGED, converged = 0, and
 * cdfem_last_error names it.  Multi-rank: none / Jacobi on slabs, ILU(0) on a general partition.
 * After a BiCGStab solve cdfem_kernel_bytes(CDFEM_K_UPDATE) is the traffic of one iteration's five
 * vector kernels and cdfem_kernel_name(CDFEM_K_UPDATE) is "k_bcgs_v<S=0>" (they read the Mult's output
 * vector) or "k_bcgs_v<S=4p+1>" (they read the structured Mult's patch buffer, "gm_pb").
 * Returns CDFEM_ERR_NOT_CONVERGED (result filled) when max_iter is reached.                     */
typedef struct {
    int method;        /* CDFEM_CG / CDFEM_GMRES / CDFEM_BICGSTAB */
    int pc;            /* CDFEM_PC_NONE / CDFEM_PC_JACOBI / CDFEM_PC_ILU (GMRES, BiCGStab on FA operators) */
    int max_iter;
    int restart;       /* GMRES restart (PETSc default 30) */
    double rel_tol;
    double abs_tol;
    int check_every;   /* host convergence poll interval in iterations (0: default 16) */
    int print_level;
} cdfem_solver_params;

typedef struct {
    int converged;
    int iterations;
    double final_norm;
    double initial_norm;
    double seconds;    /* wall time of the Krylov loop (device-synchronised) */
} cdfem_solver_result;

int cdfem_solve(cdfem_ctx *ctx, const cdfem_solver_params *prm, const double *B, double *X,
                int where, cdfem_solver_result *res);

/* ---- nonlinear heat form and Newton solve (simplex meshes, one rank) ------------------------------
 * replaces: the ParNonlinearForm of nonlinear_convection_diffusion_1D.cpp with its NonlinearMassBEIntegrator
 * (:418-507) and NonlinearDiffusionIntegrator (:509-642), Input/input_nonlinear_1d.yaml's coefficients:
 * backward Euler for m(u) du/dt = div(a(u) grad u), a(u) = a0 + a1 (u - u_ref), m(u) = m0 + m1 (u - u_ref).
 * With u_old an L-vector on the same space, W = w_q det J and the one rule both integrators use,
 * IntRules.Get(geom, 2p + OrderW + 2) = MFEM's tabulated rule of order 2p + 2 on affine simplices
 * (CDFEM_RULE_NONLINEAR):
 *   R_i  = sum_q W [ m(u) (u - u_old) / dt phi_i + a(u) grad u . grad phi_i ] - g_i
 *   J_ij = sum_q W [ (m(u) + m1 (u - u_old)) / dt phi_i phi_j + a(u) grad phi_i . grad phi_j
 *                    + a1 phi_j (grad phi_i . grad u) ]
 * Essential dofs follow MFEM's NonlinearForm: R is zero on essential rows, J has essential rows and columns
 * eliminated with a unit diagonal, a Newton solve keeps the essential values of its initial guess.
 * cdfem_nl_setup: the coefficients, the rule tables, u_old = 0 and g = 0 (CDFEM_ERR_UNSUPPORTED on a quad / hex
 * mesh and on more than one rank).  The other calls return CDFEM_ERR_STATE before it.
 * cdfem_nl_set_old: u_old = the last step's solution (GridFunctionCoefficient u_old_coeff, :817-820).
 * cdfem_nl_set_rhs: g, the Neumann load subtracted from the residual (ShiftedResidualOperator::SetBoundaryRHS,
 * :644-669, :836); NULL sets it to zero.
 * cdfem_nl_residual: R(u) (ShiftedResidualOperator::Mult, :653-660).
 * cdfem_nl_gradient: assembles J(u) on the GPU (ParNonlinearForm::GetGradient, :662-665) into the full
 * assembly's CSR: afterwards cdfem_pa_mult, cdfem_pa_diagonal, cdfem_fa_csr and cdfem_solve act on J(u), the
 * constrained forms on the eliminated matrix.                                                          */
typedef struct { double dt, a0, a1, m0, m1, u_ref; } cdfem_nl_heat_coeffs;
int cdfem_nl_setup(cdfem_ctx *ctx, const cdfem_nl_heat_coeffs *coeffs);
int cdfem_nl_set_old(cdfem_ctx *ctx, const double *u_old, int where);
int cdfem_nl_set_rhs(cdfem_ctx *ctx, const double *g, int where);
int cdfem_nl_residual(cdfem_ctx *ctx, const double *u, double *R, int where);
int cdfem_nl_gradient(cdfem_ctx *ctx, const double *u, int where);

/* quad / hex meshes (cdfem_mesh_upload), one rank: the same form as cdfem_nl_setup, matrix-free.
 * CDFEM_ERR_UNSUPPORTED on a simplex mesh, on more than one rank and outside quads p = 1..3 and hexes p = 1, 2
 * (the orders of the simplex form); CDFEM_ERR_ARG for null coefficients or dt <= 0.  R and J v are those above;
 * the geometry is the multilinear map of the element's 2^dim vertices, evaluated at every point.
 * The rule is the same IntRules.Get(geom, 2p + OrderW + 2).  For the multilinear Qk geometry MFEM's OrderW() is
 * order * dim - 1 (1 on quads, 2 on hexes), so the rule order is 2p + 3 / 2p + 4; MFEM builds square and cube
 * rules as tensor Gauss-Legendre with (order | 1) / 2 + 1 points per direction: p + 2 on quads, p + 3 on hexes,
 * one more than the operator rule.  (Derived from MFEM's sources, not pinned against an MFEM run: DESIGN 2.)
 * CDFEM_RULE_NONLINEAR reports it: (p + 2)^2 / (p + 3)^3 points, q lexicographic with qx fastest.
 * Afterwards cdfem_nl_set_old, cdfem_nl_set_rhs, cdfem_nl_residual, cdfem_newton_solve and
 * cdfem_newton_history behave as on simplices (g any L-vector, cdfem_bdr_lf_assemble's among them).
 * cdfem_nl_gradient assembles nothing: it keeps a copy of u and makes J(u) the context's current operator, on
 * which cdfem_pa_mult (constrained 0 / 1 / 2), cdfem_pa_diagonal and cdfem_solve (CG, GMRES, BiCGStab; no
 * preconditioner or Jacobi; CDFEM_PC_ILU needs an assembled operator) act matrix-free, the constrained forms on
 * the eliminated J(u); cdfem_fa_csr keeps CDFEM_ERR_STATE.  J reads the current u_old.  While J(u) is current
 * no structured fast path runs and cdfem_kernel_name(CDFEM_K_APPLY) is "k_nl_tensor"; a later cdfem_pa_setup
 * makes the linear operator current again.                                                             */
int cdfem_nl_pa_setup(cdfem_ctx *ctx, const cdfem_nl_heat_coeffs *coeffs);

/* quad / hex meshes, one rank: the same form, rule (CDFEM_RULE_NONLINEAR) and refusals as cdfem_nl_pa_setup, with
 * the Jacobian assembled: what Input/petsc_nonlinear.opts asks for (GMRES with bjacobi / ilu on every Newton step).
 * cdfem_nl_set_old, cdfem_nl_set_rhs, cdfem_nl_residual (the matrix-free kernel), cdfem_newton_solve and
 * cdfem_newton_history are unchanged.  cdfem_nl_gradient(u), and every Jacobian rebuild of cdfem_newton_solve,
 * assembles J(u) on the GPU into the full assembly's CSR of this mesh (cdfem_fa_setup's pattern, gather,
 * elimination and SELL copy; the element matrices are the formula above on the multilinear map).  Afterwards
 * cdfem_pa_mult (constrained 0 / 1 / 2), cdfem_pa_diagonal, cdfem_fa_csr and cdfem_solve act on the assembled
 * matrix, the constrained forms on the eliminated one; cdfem_solve takes CG, GMRES and BiCGStab with no
 * preconditioner, Jacobi or CDFEM_PC_ILU, and cdfem_kernel_name(CDFEM_K_APPLY) names the SpMV.
 * The assembled J is a snapshot of u and of the u_old set when it was assembled: a later cdfem_nl_set_old does
 * not change it until the next cdfem_nl_gradient (the matrix-free J of cdfem_nl_pa_setup reads the current
 * u_old).  Whichever of cdfem_nl_pa_setup and cdfem_nl_fa_setup was called last owns the nonlinear state; each
 * drops the other's Jacobian and an assembled linear operator.  cdfem_pa_setup, cdfem_fa_setup and
 * cdfem_nl_pa_setup called afterwards drop the assembled Jacobian as they drop an assembled linear operator; the
 * pattern is kept.  cdfem_profile_read(CDFEM_K_NL_ASSEMBLE / CDFEM_K_FA_GATHER / CDFEM_K_SELL_FILL) time the
 * three parts of a rebuild.                                                                             */
int cdfem_nl_fa_setup(cdfem_ctx *ctx, const cdfem_nl_heat_coeffs *coeffs);

/* replaces: NewtonPetscSolver::Solve (newton_petsc_solver.hpp:180-259; Input/petsc_nonlinear.opts for the
 * linear solve).  For iter = 0 .. max_iter - 1: R = residual(u), rn = ||R||_2; r0 = max(1, rn) on iteration 0;
 * converged when rn < abs_tol or rn / r0 < rel_tol (iterations = iter, the updates taken); else J(u) is
 * assembled when iter % jacobian_rebuild_freq == 0 (values < 1 count as 1), J dx = -R is solved from a zero
 * guess with `linear` (cdfem_solve's parameters and semantics), and u += dx.  A linear solve that does not
 * converge ends the Newton solve with CDFEM_ERR_NOT_CONVERGED and cdfem_last_error names the Newton iteration
 * (the reference throws, :354-362).  Leaving the loop without convergence gives iterations = max_iter,
 * converged = 0 and CDFEM_ERR_NOT_CONVERGED with the result filled.  A params field <= 0 takes the reference's
 * default: abs_tol 1e-10, rel_tol 1e-8, max_iter 20, jacobian_rebuild_freq 1.  u: the initial guess on input,
 * the solution on output.  u, R, dx and u_old stay on the device for the whole solve; per iteration the two
 * norms and the linear solver's own polls reach the host.  initial_residual = r0, initial_update_norm =
 * du0 = max(1, ||dx_0||); the *_seconds are host clocks around device-synchronised sections.
 * cdfem_newton_history: residual norm, update norm and linear iterations of every iteration of the last
 * Newton solve, the converged check included (update norm 0, linear iterations 0): the first min(cap, count)
 * entries, the count into *count (arrays may be NULL).                                                  */
typedef struct { double abs_tol, rel_tol; int max_iter, jacobian_rebuild_freq, print_level; } cdfem_newton_params;
typedef struct {
    int converged, iterations;
    double initial_residual, final_residual, final_relative_residual, initial_update_norm, final_update_norm;
    int linear_iterations;   /* summed over the Newton iterations */
    double residual_seconds, jacobian_seconds, linear_seconds;
} cdfem_newton_result;
int cdfem_newton_solve(cdfem_ctx *ctx, const cdfem_newton_params *prm, const cdfem_solver_params *linear,
                       double *u, int where, cdfem_newton_result *res);
int cdfem_newton_history(cdfem_ctx *ctx, double *res, double *upd, int32_t *lin_its, int cap, int *count);

/* ---- boundary linear form (one rank) ---------------------------------------------------------------
 * replaces: neumann_form.AddBoundaryIntegrator(new BoundaryLFIntegrator(flux_coeff), x_bdr); Assemble()
 * (nonlinear_convection_diffusion_1D.cpp:830-831, :952-954).  cdfem_bdr_set: the nbf boundary facets as (element,
 * local facet f = the facet opposite local vertex f); the facet's vertices are the element's other vertices in
 * ascending local order and its dofs come from a table over the element's local dof order, so no facet dof
 * list crosses the ABI.  The rule is BoundaryLFIntegrator's default (a = 1, b = 1: order p + 1 on the facet):
 * segments Gauss-Legendre with (p + 1) / 2 + 1 points, triangular facets MFEM's tabulated rule of order p + 1.
 * cdfem_bdr_quadrature_points: nbf * nq * dim physical coordinates, facet-major.
 * cdfem_bdr_lf_assemble: b_i = sum_q w_q (edge length | |t1 x t2|) g_q phi_i(q), g_q the nbf * nq point
 * values; b is an L-vector (what cdfem_nl_set_rhs takes).
 * Quad and hex meshes (quads p = 1..3, hexes p = 1, 2; cdfem_bdr_set needs only the mesh): the local facet is
 * f = 2 axis + side, side 0 at xi_axis = 0 and side 1 at xi_axis = 1 in the lexicographic vertex / dof convention
 * of cdfem_mesh_upload; f outside 0 .. 2 dim - 1 is CDFEM_ERR_ARG.  The facet's (p + 1)^(dim - 1) dofs are the
 * element's local dofs whose axis index is 0 or p, the lower remaining axis fastest.  The rule is the same default
 * order p + 1, which MFEM's segment and square rules meet with tensor Gauss-Legendre of n = (p + 1) / 2 + 1 points
 * per direction (derived from MFEM's sources, as the simplex rule was; not pinned against an MFEM run):
 * cdfem_bdr_rule_size gives n^(dim - 1), the lower remaining axis fastest.  cdfem_bdr_quadrature_points returns
 * the image under the element's multilinear map, which is not affine.  cdfem_bdr_lf_assemble uses the edge length
 * in 2D and |dx/ds x dx/dt| at the point in 3D (a perturbed hex face is bilinear).                        */
int cdfem_bdr_set(cdfem_ctx *ctx, int nbf, const int32_t *face_elem, const int32_t *face_local);
int cdfem_bdr_rule_size(cdfem_ctx *ctx, int *nq_per_facet);
int cdfem_bdr_quadrature_points(cdfem_ctx *ctx, double *xyz, int where);
int cdfem_bdr_lf_assemble(cdfem_ctx *ctx, const double *g_q, double *b, int where);

/* ---- HBM bandwidth probe: mode 0 read (16 B/lane), 1 read (8 B/lane), 2 copy (16 B/lane) of a
 * `bytes`-sized buffer, `reps` launches; returns achieved GB/s (bytes moved / time).
 * Modes 3-7: per-wave private 320 KiB chunks (16 B/lane), 8/16/8/4/32 loads in flight; 3, 4, 6, 7
 * limited to one wave per SIMD by an LDS reservation, 5 unrestricted.  Modes 8, 9: the same
 * per-wave work (8 / 4 loads in flight, one wave per SIMD) on an interleaved layout.  Modes 10-13:
 * mode 3 with chunks skewed by 256 B / 512 B / 1 KiB / 4 KiB.  Modes 14, 15: 4 (one workgroup per
 * CU) / 2 waves of a workgroup streaming one shared chunk, 4 / 2 KiB per step.  Modes 16, 17: the
 * 16-byte grid-stride read with 64-thread blocks at one wave per SIMD, 1024 / 4096 blocks.       */
int cdfem_stream_bench(cdfem_ctx *ctx, int mode, size_t bytes, int reps, double *gbps);

/* f64 compute-rate probe (diagnostic; backs DESIGN.md's VALU-vs-MFMA choice for the high-order
 * contractions): mode 0 = v_fma_f64 (8 independent chains per lane), 1 = v_mfma_f64_16x16x4_f64
 * (4 independent accumulators per wave), 2 / 3 / 4 = both in one loop (4 MFMA chains interleaved
 * with 16 / 32 / 64 v_fma_f64 per lane: does the matrix core run beside the VALU?);
 * *tflops = achieved f64 TFLOP/s over `reps` launches. */
int cdfem_fp64_bench(cdfem_ctx *ctx, int mode, int reps, double *tflops);

/* ---- tuning knobs (performance only; results identical to rounding) --------------------------
 * "profile_mask": bit k set = kernel slot k (CDFEM_K_*) gets HIP events while profiling is on
 *                 (default all; events around every kernel cost ~1 us each on the stream).
 * "brick_xcd": 1 (default) — XCD-contiguous brick order of the structured CG kernel; 0 = the
 *              dispatcher's round-robin order.
 * "mr_overlap": 1 (default) — slab (multi-rank) structured CG: the first/last brick layers, the
 *               interface pack and the exchange run on a side stream under the interior layers;
 *               0 = one launch, then the exchange (bitwise the same results).
 * "brick_mult_pb": 1 (default) — the structured Mult (GMRES, cdfem_pa_mult; Kronecker form) writes
 *              each brick's whole patch sum to the patch buffer and a second pass forms every row from
 *              its 1-8 entries (predicated loads); 0 = owned rows + face partials + face sums
 *              (k_brick_faces).  Same sums in the same order (bitwise); C2 GMRES step 195.0 -> 189.4 us,
 *              profiles/r04/ab_c2_gmres_dpp_multpb.json.
 * "cg_beta_fold": 1 (default) — with cg_den_fold (one rank, Kronecker form, <= 1024 update
 *              workgroups) the brick CG apply also takes MFEM's betanom step of the previous update:
 *              every workgroup sums the update's partials with its patch gather in flight, and the
 *              one-block update finalizer is not launched (iterates agree with 0 to rounding; C2:
 *              60.8 against 62.6 us per iteration, profiles/r04/ab_c2_beta_fold.json).
 * "cg_beta_sum": 0 (default) — 1: with cg_beta_fold on one rank, before the uniform-box apply (pa_uniform), the
 *              update's last-arriving workgroup (an agent-scope arrival count with release / acquire, no
 *              waiting) sums the betanom partials once, in the order every apply workgroup would, and the apply
 *              loads that one double (bitwise the same iterates).  Off: the release in each of C2's 1,024
 *              update workgroups costs 23 us per iteration (profiles/r14/ab_c2_one_round/).  The Kronecker-form
 *              apply and several ranks always read the vector.
 * "cg_den_fold": 1024 (default) — N (64..16384): the one-rank brick CG takes MFEM's den step inside
 *              the update kernel, run as N workgroups that each sum the apply's den partials in one
 *              fixed order; the one-block den finalizer is not launched (iterates agree with the
 *              finalizer path, 0, to rounding; C2: 62.4 against 64.6 us per iteration,
 *              profiles/r04/ab_c2_den_fold.json).
 * "cg_mr_fold": 1 (default) — several ranks (slab partition, p <= 2, both folds on): the ranks
 *              all-reduce the apply's den partials and the update's betanom partials as vectors, so the
 *              update and the next apply take MFEM's den and betanom steps as on one rank (no sum or
 *              step kernels between them); taken only when every rank holds as many partials (checked
 *              once, collectively); 0 = per-rank sums, 8-byte all-reduces and step kernels.
 * "gm_poll": 4 (default) — the GMRES host loop records an event and checks the device state every k
 *              inner steps (and at every cycle's last step) instead of after every step (1: every step).
 *              Steps queued past a converged step exit at entry; their Mult runs (at most 2k - 1 per solve).
 * "brick_stagger": -1 (default, automatic: s = log2 CUs, n = 4), 0 off, or bits 0-3 a shift s and bits
 *              4-8 a count n: the first round of the brick CG apply (k_brick_cg workgroups b < 8 x CUs,
 *              launches of >= 2 rounds) with bit s of b set sleeps n x 2,048 cycles at entry, so half the
 *              round gathers its patches while the other half computes (C2: 39.0 -> 37.4 us per apply,
 *              DESIGN.md 4.1).
 * "pa_uniform": 1 (default) — under pa_affine 2 on a structured p = 2 box (kinds 7 or 5), cdfem_pa_setup
 *              checks whether every element's factors equal the first element's (each within 1e-14 of the
 *              largest factor: a uniformly refined box, what MFEM's MakeCartesian3D gives) and, if so,
 *              forms that element's 27 x 27 matrix once (column j = the Kronecker apply of e_j); the brick
 *              CG apply then runs it as a GEMM on the matrix cores (56 v_mfma_f64_16x16x4_f64 per 64
 *              elements; the same operator to rounding).  0 = the Kronecker form (takes effect without a
 *              new setup; 1 needs one).  The GMRES Mult and the other applies keep the Kronecker form.
 * "pa_uniform_diag": 1 (default) — where pa_uniform's matrix is in use, the Jacobi scale of such a box takes 64
 *              values (per axis a lattice coordinate is element-interior, shared by two elements, on the
 *              first plane or on the last; essential dofs take 1).  When the scale is formed, the library
 *              fills that table from it (a class's entry = the vector's at the class's lowest non-essential
 *              lattice index) and checks the vector against it on the device (1e-14 relative, essential
 *              entries exactly 1; several ranks: on every rank).  If the check passes, the Jacobi-CG apply
 *              and update of the brick path read the table from LDS instead of streaming the vector (17 MB
 *              less per kernel and iteration at 64^3; the iterates agree to rounding).  0 =
 *              stream the vector; read at solve time.  pc = none, GMRES and every other path keep the vector.
 * "ho_uniform": 0 (default) or 1 — the same for the high-order block CG, read by cdfem_pa_setup.  With 1
 *              the setup checks whether every element's factors equal element 0's, each component within
 *              1e-14 of its own magnitude, and, if so, forms that element's N x N matrix once (N = 64 at
 *              p = 3, 125 at p = 4; column j = the Kronecker apply of e_j).  The check is taken when all of
 *              these hold: a structured 3D box at p = 3 or 4 with the operators' rule (q1 = 5, 6); kinds 7
 *              or 5; pa_affine 2 on the high-order tile layout; one rank; the block CG ("ho_brick") on
 *              2 x 2 x 4 blocks ("ho_block_z" 4, whose 16 elements are the 16 columns of one
 *              v_mfma_f64_16x16x4_f64 tile).  The CG apply is then k_hobrick_um: a persistent kernel whose
 *              waves each hold a 16-row tile of the matrix in registers and form Y (N x 16) = A X per block
 *              on the matrix cores (the same operator to rounding; elements of a partial block outside the
 *              box are masked).  In every other case (not uniform, other kinds, 2^3 blocks, several ranks,
 *              per-point data) the setup keeps the Kronecker form without a word.  0 after a setup switches
 *              back without a new setup; 1 needs one.  The GMRES Mult and the other applies keep the
 *              Kronecker form.  Measured on C3 (profiles/r07/ab_c3_ho_uniform/): level with
 *              the Kronecker form on the same blocks, 20 % behind the default 2^3 blocks on the apply.
 * "ho_uniform_grid": 0 (default, automatic: what a CU holds at once, one 8-wave workgroup at p = 4 and two
 *              of 4 waves at p = 3, times the CUs, at most one workgroup per block) or the number
 *              of k_hobrick_um workgroups (tests: a small box walked by few workgroups with an uneven
 *              remainder).  The iterates do not depend on it, bitwise.
 * "brick_mfma": 0 (default) or 1 — the p = 2 brick CG apply's x stage (kinds 7, Kronecker form) on
 *              v_mfma_f64_16x16x4_f64: 16 elements per GEMM, outputs staged through LDS to the element
 *              threads.  Parity-green, measured slower.
 * "ho_block_z": 2 (default) or 4 — elements per block along z of the high-order brick CG (read by
 *              cdfem_mesh_set_structured): 2 x 2 x 2 blocks (8 element tiles, 200 of 256 threads busy at
 *              p = 4) or 2 x 2 x 4 (16 tiles, 400 of 448; 1.34 patch entries per dof against 1.42).
 * "ho_brick": 1 (default) — the CG solve on a structured affine box at 3D p = 3, 4 (one rank,
 *              Kronecker form) runs on blocks of 2^3 elements (k_hobrick_cg: the tile core, the block's
 *              E->L in LDS, the 9^3 patch buffer of the p = 2 brick) and the brick update, instead of the
 *              tile apply's E-vector and the flat E->L update (0).  Iterates agree to rounding; C3:
 *              4114 against 4287 us per iteration (profiles/r05/ab_c3_ho_brick_occ4.json).
 * "ho_brick_mfma": 0 (default) — with ho_brick on the full operator (kinds 7): the x stage of the
 *              block's eight elements as GEMMs on v_mfma_f64_16x16x4_f64 (rows = element rows, k = the
 *              five input points padded to eight, columns = M, K, C, C^T per output point), staged to
 *              the tile threads through LDS; the y and z stages stay on the VALU.  Same operator to
 *              rounding; the north star's MFMA contraction, A/B'd in DESIGN.md 4.2.
 * "den_group": 0 (default) — on several ranks the brick CG apply's den partials (one per 64-element brick)
 *              are summed in groups by the group's last-arriving brick once there are more than the
 *              multi-rank fold sums (8,192: C5's per-rank slab of 32,768 bricks -> groups of 8), so the
 *              fold stays on; one rank keeps per-brick partials (measured: its 256^3 box runs the
 *              two-stage den sum 0.3 % faster); a power of two up to 64 forces that size (tests).
 * "brick_byte_limit": 2^31 (default) — the structured brick kernels address their vectors and patch
 *              buffer with 32-bit buffer offsets (out-of-range marker 2^31), so a box whose 8 N_L or
 *              8 S^3 bricks reach the limit runs the generic element kernels instead; lower values
 *              force that fallback (tests); 0 restores the default.  On a slab partition the
 *              decision is taken on the largest rank's sizes (all-reduced by cdfem_set_slab), so
 *              every rank runs the same CG path.
 * "brick_upd_pb": 1 (default) — the brick CG update (k_cg_update_faces) reads each dof's 1-8 patch
 *              entries as eight predicated buffer loads (absent ones out of range) instead of
 *              branching on the face planes (0); bitwise the same sums.
 * "ho_dfold": 1 (default) — read by the CG solve on structured boxes (one rank, fused high-order CG,
 *              Kronecker tile: pa_affine 2, ho_mfma 0): the apply gathers z and the previous
 *              direction, forms d = z + beta d_old itself (each dof's owner element stores it to a
 *              second direction buffer), and the direction pass is skipped (same formula); 0 = the
 *              direction pass.
 * "ho_mfma": 0 (default) — the LDS stages of the high-order (3D p = 3, 4) tile apply as block GEMMs on
 *            v_mfma_f64_16x16x4_f64, bit 0 = stage x, 1 = y, 2 = y^T, 3 = x^T; the masks 1, 3, 8, 9
 *            and 15 are built (results agree to rounding; the north star's MFMA alternative,
 *            measured even to slower).
 * "pa_affine": 2 (default) — read by cdfem_pa_setup: on a mesh whose elements are all
 *              parallelepipeds (checked at upload: every vertex within 32 ulp of the coordinates plus
 *              1e-12 of the element's longest edge of v0 + sum of the edge vectors) with constant
 *              coefficients, the Jacobian is the element's edge matrix, the per-point data are stored
 *              as W_q * g_e (so the diagonal and the 2D / FA paths see the same operator), and the
 *              3D applies read the 10 per-element factors g_e instead of the per-point stream:
 *                2 — the structured brick kernels (p <= 2, CG and Mult) and the generic 3D
 *                    element-block apply (p <= 2) apply the factors in their Kronecker form
 *                    (1D rule matrices M, K, C per axis, pa_core.hpp elem_apply3d_kron);
 *                1 — the same applies form each point's data W_q * g_e from the factors;
 *                the p >= 3 tile apply forms the point data from the factors under 1 and 2 (and
 *                streams them when "ho_mfma" is non-zero).  The 2D applies always stream the per-point
 *                data.  All forms apply the operator of the per-point multilinear-map setup to rounding
 *                (the Kronecker form is an algebraic identity of the tensor rule, not an exactness
 *                argument); 0 = the per-point map and stream everywhere.
 * "pa_geom": 0 (default) or 1 — read by cdfem_pa_setup: geometric factors formed inside the apply on hex
 *              meshes the affine forms do not take (a perturbed box, a moved mesh).  With 1 the setup keeps,
 *              next to the per-point stream, 22 doubles per element (a padding mask and the coefficients
 *              a1..a7 of the element's trilinear map, 176 B against the stream's 5,120 B at p = 2, kinds 7),
 *              and the 3D p <= 2 applies — the generic element-block apply k_apply3d, the structured Mult
 *              k_brick3d (GMRES, cdfem_pa_mult) and the structured CG apply k_brick_cg, on one rank or on
 *              slabs — form J, adj(J), det J and D = W kappa adj(J) adj(J)^T / det J, C = W alpha adj(J) c,
 *              M = W s det J in registers at every point (pa_core.hpp elem_apply3d<..., GEO>; the operator of
 *              the stream to rounding, one division per point).  Taken when all of these hold: hex mesh,
 *              dim 3, p = 1 or 2 with the operators' rule (q1 = p + 2); every coefficient constant (kappa_q,
 *              kappa_mat_q, conv_q and mass_q all NULL); the affine form not taken (mesh not affine, or
 *              "pa_affine" 0).  On an affine mesh with pa_affine != 0 the Kronecker form stays, and in every
 *              other case (per-point coefficients, p = 3, 4: the high-order tile kernels, 2D) the setup keeps
 *              the stream without a word.  The stream is still allocated and filled (the diagonal,
 *              FormLinearSystem and the 2D paths read it), so 0 after a setup switches back without a new
 *              setup; 1 needs one.  The kernels run with the stream's launch structure (one wave per SIMD, no
 *              CG folds), 476 registers at p = 2 kinds 7 without scratch.  The MFEM-shaped C++ layer
 *              (cpp/cdfem_mfem.hpp) has no option channel and keeps the default.
 *              Measured on the perturbed C2 box (64^3, p = 2, perturb 0.1; tools/ab_geom.py, DESIGN.md 4.1,
 *              profiles/r08/ab_c2_geom_fly/), pa_geom 1 against 0 on the same box in one process, kinds 7:
 *              CG apply 95.4 against 240.6 us, CG 1.39e10 against 7.14e9 DoF-iter/s, GMRES(30) 9.05e9 against
 *              5.98e9; apply bytes 140.9 MB against 1,436.9 MB, flops 3.12 G against 1.85 G (32.7 TFLOP/s,
 *              0.42 of the f64 peak: the apply is VALU-bound).  Kinds 5: apply 92.9 against 178.1 us, CG
 *              1.43e10 against 9.04e9.  Iterates agree to 3e-15.  Not measured: the generic element-block
 *              apply, p = 1, several ranks (parity-tested only), and no counter pass was taken.  The p = 3, 4
 *              tile apply has its own option of the same kind, "ho_geom".
 * "ho_geom": 0 (default) or 1 — read by cdfem_pa_setup: the same for the high-order tile apply.  With 1 the
 *              setup keeps, next to the per-point stream, 24 doubles per element, element-major (the
 *              coefficients a1..a7 of the trilinear map, the same values pa_geom keeps, and 3 zeros: 192 B
 *              against the stream's 17,280 B at p = 4, kinds 7), and k_apply3d_tile (mode bit 32) forms the
 *              point operator itself: thread (qx, qy) hoists the parts of J that are fixed along its column of
 *              points (15 doubles and w_x w_y instead of the stream's Q1 * nc) and per plane qz forms the two
 *              remaining columns of J, adj(J), det J and applies D, C, M in their factors exactly as
 *              pa_core.hpp elem_apply3d<..., GEO> (the operator of the stream to rounding, one reciprocal per
 *              point).  Taken when all of these hold: hex mesh, dim 3, p = 3 or 4 on the operators' rule
 *              (q1 = p + 2); every coefficient constant (kappa_q, kappa_mat_q, conv_q and mass_q all NULL); the
 *              affine forms not taken (mesh not affine, or "pa_affine" 0); "ho_mfma" 0 (read when the apply
 *              runs: the matrix-core stage variants keep the stream).  Every other case (p <= 2, 2D, per-point
 *              coefficients, an affine mesh under pa_affine != 0) keeps its form without a word.  Mult, GMRES,
 *              the fused and the unfused CG, generic meshes (the map gather), slabs and the general partition
 *              take it wherever they run the stream tile; the launch structure is the stream's.  The stream is
 *              still allocated and filled (the diagonal, FormLinearSystem and the linear form read it), so 0
 *              after a setup switches back without a new setup; 1 needs one.  126-154 registers at kinds 7
 *              (three waves per SIMD against the stream's two at 226-241), no scratch; a __launch_bounds__
 *              (256, 3) gives the same register counts, so there was nothing to A/B.  The MFEM-shaped C++ layer
 *              keeps the default.
 *              Measured on the perturbed C3 box (128^3, p = 4, perturb 0.1, 135.0 M dofs; tools/ab_geom.py
 *              --option ho_geom --p 4, DESIGN.md 4.2, profiles/r09/ab_c3_ho_geom/), ho_geom 1 against 0 on the
 *              same box in one process, kinds 7: apply 4,176 against 7,123 us, CG 1.98e10 against 1.40e10
 *              DoF-iter/s, GMRES(30) 1.09e10 against 8.52e9; apply bytes 3.71 GB against 39.55 GB, flops 115.5 G
 *              against 81.4 G (27.7 TFLOP/s, 0.35 of the f64 peak: the apply has left the HBM bound).  Kinds 5:
 *              apply 4,128 against 5,701 us, CG 2.00e10 against 1.65e10.  Iterates agree to 4.0e-15.  On 64^3:
 *              apply 530.9 against 897.1 us, CG 1.96e10 against 1.37e10.  Not measured: p = 3, the generic (map
 *              gather) path, several ranks (parity-tested only), and no counter pass was taken.
 * "cg_xfold": 1 (default) — structured brick CG (p <= 2, Kronecker form): each apply after the first
 *             advances x by the previous iteration's alpha d on the dofs it writes the new direction
 *             for, so the update kernel streams neither x nor d (bitwise the same iterates; 1 % faster
 *             at C2 in two A/B runs, profiles/r04/ab_c2_patchbuf_xfold.json, ab_c2_xfold_pb.json);
 *             0 = x += alpha d in the update.
 * "cg_fused": 1 (default) — high-order (p = 3, 4) CG on a structured box, one rank: (d, A d) from the
 *             apply's element outputs and the E->L sum fused into the CG update; 0 = separate
 *             E->L kernel (results agree to rounding).
 * "spmv_index16": 1 (default) — the assembled-operator SpMV streams 16-bit column deltas
 *                 (column - lane row); a 64-row slice with a delta beyond 2^15 streams its 32-bit
 *                 columns instead (mixed layout, when at least half the entries fit); 0 = 32-bit
 *                 columns everywhere.
 * "sell_order": 0..8, default 8 — the FA SpMV's order, read when the pattern is built
 *               (cdfem_fa_setup on a new mesh; see cdfem_sell_plan): 0 natural, 1 natural +
 *               windows, 2 RCM + windows, 3 auto (banded mesh order, geometric, RCM), 4 RCM, 5
 *               geometric, 6 Morton + windows, 7 Morton, 8 Morton windows of 768 rows staged in LDS
 *               (2 or 4 lanes per row by the padding) when the dof coordinates are known, else 3.
 *               A permuted order runs the Krylov solve in that order (Mult to rounding, iterates to
 *               1e-12).
 * "sell_window": 0 (default, auto) or a multiple of 64 — rows per window of the windowed orders.
 * "spmv_lpr": 0 (default, auto), 1, 2 or 4 — lanes per row of the LDS-staged layouts (read when
 *             the pattern is built): each lane sums a contiguous part of its row and the parts are
 *             combined in a fixed order (less padding where row lengths vary; results to rounding);
 *             auto = 4 where one lane per row would pad slices by more than 15 %, else 2, on the
 *             auto modes' LDS layouts; 1 elsewhere.
 * "spmv_lds": -1 (default, auto), 0 or rows per window — LDS-staged SpMV windows for the windowed
 *             orders: each workgroup stages its window's distinct columns in LDS and the entries
 *             address them by 16-bit window positions (bitwise the windowed sums); auto = on for the
 *             auto orders (sell_order 8, and the RCM windows sell_order 3 picks on unstructured meshes
 *             without coordinates: 768 rows).
 * "spmv_xcd": 1 (default) — contiguous slice range per XCD for the windowed SpMV layout.
 * "gm_ept": 0 (default, auto) — entries per thread of the GMRES orthogonalisation passes (4, 5, 6
 *           or 8); auto takes the smallest whose grid is resident in one round (same results).
 * "gm_pb": 1 (default) — GMRES and BiCGStab on the structured patch-buffer Mult (one rank, Jacobi
 *          or no preconditioner): the kernel that takes the Mult's result (GMRES's first
 *          orthogonalisation pass, BiCGStab's k_bcgs_v / k_bcgs_t) sums each row's patch entries itself,
 *          so the Mult's row-sum kernel and its output vector's write and re-read go away (same sums in
 *          the same order: bitwise the same iterates); 0 = the Mult's own row sums.
 * Variants measured slower and removed in round 3 (their records stay under profiles/r02_ab_*):
 * brick element cores 1-10 and the four-waves-per-brick kernel, x-fold / paired x updates, the
 * folded high-order direction, the derived mass weight, per-XCD SpMV sort, SpMV stream offsets and
 * the software-pipelined SpMV loop, the two-waves-per-SIMD structured Mult, 2 / 4 lanes per SpMV row
 * (profiles/r03/ab_c4_spmv_lanes_per_row.txt), a spinning / less frequent GMRES host poll
 * (profiles/r03/ab_c2_gmres_poll.txt), in-launch grid sums for the CG / GMRES scalars
 * (profiles/r03/ab_c2_grid_fin.txt), brick-face sums in GMRES pass 1
 * (profiles/r03/ab_c2_gmres_faces_pass1.txt), chunked SELL storage with wide loads
 * (profiles/r03/ab_c4_spmv_chunk.txt), XCD-ordered blocks of the p >= 3 tile apply
 * (profiles/r03/ab_c3_tile_xcd_order.txt).                                                         */
int cdfem_set_option(cdfem_ctx *ctx, const char *key, int value);

/* ---- profiling (live HIP-event timing of the hot kernels, on the context's stream) ------------ */
int cdfem_profile_enable(cdfem_ctx *ctx, int on);
int cdfem_profile_reset(cdfem_ctx *ctx);
/* total milliseconds and launch count of kernel id (CDFEM_K_*) since the last reset */
int cdfem_profile_read(cdfem_ctx *ctx, int kernel, double *total_ms, int64_t *count);
/* per-launch milliseconds of kernel id since the last reset, in launch order: the first min(cap, count)
 * into ms, the count into *count (bench.py separates the full launches from the early-return ones) */
int cdfem_profile_launches(cdfem_ctx *ctx, int kernel, double *ms, int64_t cap, int64_t *count);
/* algorithmic bytes moved by one launch of kernel id (see DESIGN.md for the per-unit figures); on
 * structured boxes the figure is that of the kernel the CG solve launches (the brick CG kernels, the
 * fused high-order apply with its direction fold); under pa_geom the apply's 176 B of geometry per
 * element (under ho_geom 192 B) replace the per-point stream's 8 nq nc                             */
int cdfem_kernel_bytes(cdfem_ctx *ctx, int kernel, double *bytes);
/* algorithmic f64 flops of one launch of the 3D partial-assembly apply (CDFEM_K_APPLY; FMA = 2):
 * the sum-factorized element apply (plus the point data W_q * g_e under pa_affine 1, or the point
 * operator formed from the element's trilinear map under pa_geom or ho_geom, its reciprocal counted as 1), or
 * the Kronecker-form element apply under pa_affine 2                             */
int cdfem_kernel_flops(cdfem_ctx *ctx, int kernel, double *flops);
/* the HIP kernel name (without template arguments) kernel id runs as in the current configuration,
 * as rocprof reports it: the operator apply of a CG solve (CDFEM_K_APPLY) only — the SpMV after
 * cdfem_fa_setup, else the partial-assembly apply of the path the context takes (brick CG, the
 * high-order block CG, the tile applies, the element-block apply)                                  */
int cdfem_kernel_name(cdfem_ctx *ctx, int kernel, char *buf, size_t n);

/* ---- multi-GPU (element-partitioned z-slabs, one context per GPU / rank) ----------------------
 * replaces: MPI_COMM_WORLD + ParMesh partition (linear_convection_diffusion_2D.cpp:300) and the MPI
 * traffic inside hypre/PETSc (halo sums, Krylov all-reduces).  Each rank uploads its slab
 * (cdfem_box_mesh with [z0,z1)), declares it structured, then attaches a communicator and marks
 * which of its z-end planes are shared with a neighbour (the lower rank owns a shared plane).
 * Backends: RCCL (stream-ordered, over xGMI) or host callbacks (any transport: gloo, MPI).      */
typedef int (*cdfem_allreduce_fn)(double *buf, int n, void *user);  /* in-place sum over ranks */
/* send_lo -> rank-1, recv_lo <- rank-1, send_hi -> rank+1, recv_hi <- rank+1 (NULL if absent) */
typedef int (*cdfem_exchange_fn)(const double *send_lo, double *recv_lo, const double *send_hi,
                                 double *recv_hi, int64_t n, void *user);
int cdfem_comm_unique_id(unsigned char *id /* 128 bytes */);
int cdfem_comm_init_rccl(cdfem_ctx *ctx, int rank, int nranks, const unsigned char *id);
int cdfem_comm_init_host(cdfem_ctx *ctx, int rank, int nranks, cdfem_allreduce_fn allreduce,
                         cdfem_exchange_fn exchange, void *user);
int cdfem_set_slab(cdfem_ctx *ctx, int zlo_shared, int zhi_shared);

/* General element partition of any conforming mesh (ParMesh(MPI_COMM_WORLD, *mesh) and the
 * ParFiniteElementSpace shared-dof groups, linear_convection_diffusion_2D.cpp:300,312; used where the
 * mesh is not a structured box, e.g. the reference's gmsh triangles).  After uploading its local mesh
 * and attaching a communicator, each rank lists per neighbour rank (strictly ascending) the local dofs
 * it shares with that rank, in the same order on both sides (ascending global id).  A shared dof is
 * OWNED by the lowest rank holding it, and the local numbering must list the dofs owned by lower ranks
 * first: the true dofs are the suffix of the L-vector (cdfem_local_space produces this numbering).
 * Shared sums add every holder's partial in ascending rank order, so all copies are bitwise equal.
 * nbr_off: n_nbr + 1 offsets into nbr_idx (n_nbr = 0: a rank that shares nothing).                 */
int cdfem_set_shared(cdfem_ctx *ctx, int n_nbr, const int32_t *nbr_ranks, const int64_t *nbr_off,
                     const int32_t *nbr_idx);
/* Collective between neighbours, after cdfem_set_shared: sends the global id (l2g, nl entries) of
 * every shared entry and checks that each neighbour's list holds the same id at the same position
 * (the shared sums pair entries by position).  CDFEM_ERR_ARG on a mismatch, on both ranks of the
 * pair, naming the neighbour and the first differing entry.                                     */
int cdfem_check_shared(cdfem_ctx *ctx, const int64_t *l2g);
/* Host backend of the general partition: send[nbr_off[k] .. nbr_off[k+1]) goes to nbr_ranks[k] and
 * recv[same range] receives from it (MPI_Isend/Irecv, gloo, ...).  RCCL contexts need none.      */
typedef int (*cdfem_nbr_exchange_fn)(int n_nbr, const int32_t *nbr_ranks, const int64_t *nbr_off,
                                     const double *send, double *recv, void *user);
int cdfem_comm_set_host_nbr_exchange(cdfem_ctx *ctx, cdfem_nbr_exchange_fn fn, void *user);
/* dst uses src's communicator (reference counted): every form of one ParFiniteElementSpace is its
 * own context, and they share one RCCL communicator instead of bootstrapping one each.          */
int cdfem_comm_share(cdfem_ctx *dst, const cdfem_ctx *src);

/* True dofs (MFEM T-vector) = the owned L-dofs, the suffix [first_owned, nl) of the L-vector
 * (slab: the lower interface plane belongs to the rank below; one rank: everything).
 * replaces: ParFiniteElementSpace::TrueVSize / GetTrueDofs (:313,353).                          */
int cdfem_true_size(cdfem_ctx *ctx, int64_t *ntrue, int64_t *first_owned);
/* x = P X: the L-vector (nl) of the true-dof vector X (ntrue): owned entries from X, the other
 * shared entries received from their owner.  replaces: RecoverFEMSolution's P (:377).           */
int cdfem_prolongate(cdfem_ctx *ctx, const double *X, double *x, int where);

/* Communicator report: "backend=<none|rccl|host> rccl_version=<ncclGetVersion> rccl_path=<file>",
 * the RCCL build libcdfem.so is bound to in this process (ctx may be NULL).                      */
int cdfem_comm_info(const cdfem_ctx *ctx, char *buf, size_t n);

/* ---- structured mesh helper (host only, no device needed) ---------------------------------------
 * Box [0,1]^dim into nx*ny(*nz) quads/hexes with the conventions above; rank-slab variant for
 * the element-partitioned multi-GPU path: elements with iz in [z0, z1) only, dofs renumbered
 * locally (L-vector of the slab).  Sizes: see cdfem_box_sizes.                                 */
int cdfem_box_sizes(int dim, int nx, int ny, int nz, int order, int z0, int z1, int *ne,
                    int64_t *nldofs, int *n_ess);
int cdfem_box_mesh(int dim, int nx, int ny, int nz, int order, int z0, int z1, double perturb,
                   double *elem_verts, int32_t *elem_dofs, int32_t *ess_dofs, double *dof_xyz);

/* Kuhn simplex mesh of [0,1]^dim (config C4): n^dim cubes, dim! simplices each, P1/P2 dofs on the
 * (order n + 1)^dim lattice; perturb moves interior vertices (returns CDFEM_ERR_ARG if that inverts
 * an element).  Host only.                                                                      */
/* Element partition for the general path (host only): recursive coordinate bisection of the element
 * centroids into nranks parts, part[e] = rank (MFEM's ParMesh calls METIS, which is absent here; any
 * partition defines the same global operator).  Deterministic: every rank computes the same one.  */
int cdfem_partition_rcb(int dim, int ne, int nv, const double *elem_verts, int nranks, int32_t *part);
/* Order of the assembled operator's SpMV (host only; what cdfem_fa_setup builds with set_option
 * "sell_order" = mode: 0 mesh order + global length sort, 1 natural + windows, 2 reverse
 * Cuthill-McKee + windows, 3 auto (the mesh order when banded, else the geometric order when xyz is
 * given and banded, else RCM + global when it halves the bandwidth), 4 RCM + global, 5 geometric +
 * global).  xyz: nl * dim dof coordinates or NULL (cdfem_fa_setup passes the space's nodes: the simplex
 * space's, or the multilinear map at the GLL nodes on quads and hexes).
 * perm[space row] = mesh row; info[0..6] = base order (1 natural, 2 RCM, 3 geometric), window rows
 * (0: global length sort), max |column - row| in the space order, natural bandwidth, RCM bandwidth
 * (0 if not computed), stored SELL entries / nnz * 1e6, geometric bandwidth (0 if not computed).
 * Internal layout choice with no reference counterpart (the reference multiplies in mesh order,
 * PETSc MatMult on MATAIJ); exported for tests and tools.  */
int cdfem_sell_plan(int64_t nl, const int32_t *rowptr, const int32_t *cols, int mode, int dim, const double *xyz,
                    int32_t *perm, int64_t *info);
/* The rank-local H1 space of a partition (host only): elems = the rank's elements (ascending global
 * index), loc_dofs = their dofs in local numbering (dofs owned by lower ranks first, then the owned
 * ones, each by ascending global id), l2g = global id of each local dof, and the neighbour lists that
 * cdfem_set_shared takes.                                                                        */
int cdfem_local_space_sizes(int ne, int nd, int64_t nldofs, const int32_t *elem_dofs, const int32_t *part,
                            int rank, int *ne_loc, int64_t *nl_loc, int *n_nbr, int64_t *n_shared,
                            int64_t *n_not_owned);
int cdfem_local_space(int ne, int nd, int64_t nldofs, const int32_t *elem_dofs, const int32_t *part, int rank,
                      int32_t *elems, int32_t *loc_dofs, int64_t *l2g, int32_t *nbr_ranks, int64_t *nbr_off,
                      int32_t *nbr_idx);

int cdfem_kuhn_sizes(int dim, int n, int order, int *ne, int64_t *nldofs, int *n_ess);
int cdfem_kuhn_mesh(int dim, int n, int order, double perturb, double *elem_verts, int32_t *elem_dofs,
                    int32_t *ess_dofs, double *dof_xyz);

/* gmsh v2.2 ASCII simplex meshes (the reference's inputs, e.g. Mesh/unit_square.msh); replaces
 * Mesh(mesh_file, 1, 1) + H1_FECollection(order, dim) + ParFiniteElementSpace
 * (linear_convection_diffusion_2D.cpp:290,311-313).  Triangles (order 1-3) in MFEM's vertex order
 * (Finalize: orientation fix, then the longest edge first, Triangle::MarkEdge) or tetrahedra (1-2,
 * re-oriented to det J > 0); dofs: vertices (increasing gmsh node id), then (order-1) per edge (edges
 * numbered as MFEM first meets them) along increasing vertex dof, then P3 triangle centroids.
 * Boundary physical tags must be 1..31 (a larger tag is an error).  dof_bdr_mask[i] has bit (a-1) set when dof i
 * lies on a boundary element of physical attribute a (GetEssentialTrueDofs with an ess_bdr marker).
 * Host only; the element arrays feed cdfem_mesh_upload_simplex.                               */
int cdfem_gmsh_sizes(const char *path, int order, int *dim, int *ne, int64_t *nldofs);
int cdfem_gmsh_mesh(const char *path, int order, double *elem_verts, int32_t *elem_dofs, int32_t *dof_bdr_mask,
                    double *dof_xyz);
/* The same in two steps, for callers that refine or partition the mesh first (Mesh /
 * UniformRefinement / ParMesh, linear_convection_diffusion_2D.cpp:290-305): the gmsh file's simplex
 * topology (vertices in increasing node id, xyz nvert*dim; domain elements ne*(dim+1) vertex indices;
 * boundary elements nbe*dim vertex indices with their physical tags), and the H1 space of order p on
 * any such topology (the arrays of cdfem_gmsh_mesh; boundary masks from the tagged boundary
 * elements).  Host only.                                                                        */
int cdfem_gmsh_topology_sizes(const char *path, int *dim, int64_t *nvert, int *ne, int *nbe);
int cdfem_gmsh_topology(const char *path, double *vxyz, int32_t *elem_v, int32_t *bdr_v, int32_t *bdr_attr);
int cdfem_simplex_space_sizes(int dim, int64_t nvert, const double *vxyz, int ne, const int32_t *elem_v, int order,
                              int64_t *nldofs);
int cdfem_simplex_space(int dim, int64_t nvert, const double *vxyz, int ne, const int32_t *elem_v, int nbe,
                        const int32_t *bdr_v, const int32_t *bdr_attr, int order, double *elem_verts,
                        int32_t *elem_dofs, int32_t *dof_bdr_mask, double *dof_xyz);

/* Host helpers: the collapsed-Gauss simplex rule (returns the point count; xi/w may be NULL to
 * query it) and the nodal simplex basis phi [npts][nd], dphi [npts][nd][dim] in the local dof
 * order above — for host-side functionals (ComputeL2Error, :383-392).                         */
int cdfem_simplex_rule(int dim, int n, double *xi, double *w);
/* The rule IntRules.Get(TRIANGLE / TETRAHEDRON, order) returns in MFEM: its tabulated symmetric rules
 * (triangles order <= 9, tetrahedra order <= 6; tools/simplex_rules.py), else a collapsed-Gauss rule
 * exact to that order.  Returns the point count (xi / w may be NULL to query it).  The linear-form
 * rule of cdfem_mesh_upload_simplex is this rule at order 2p (DomainLFIntegrator's default).     */
int cdfem_simplex_rule_order(int dim, int order, double *xi, double *w);
int cdfem_simplex_basis(int dim, int order, int npts, const double *xi, double *phi, double *dphi);

#ifdef __cplusplus
}
#endif
#endif /* CDFEM_H */
