// nl_kernels.hip — the quasi-linear backward-Euler heat form on affine simplices (the reference's
// nonlinear_convection_diffusion_1D.cpp:418-642: NonlinearHeatIntegrator's AssembleElementVector and
// AssembleElementGrad) and the boundary linear form of its Neumann data (BoundaryLFIntegrator, :644-669).
//
//   a(u) = a0 + a1 (u - u_ref),  m(u) = m0 + m1 (u - u_ref),  W = w_q det J, one rule of order 2p + 2:
//   R_i  = sum_q W [ m(u) (u - u_old) / dt phi_i + a(u) grad u . grad phi_i ]
//   J_ij = sum_q W [ (m(u) + m1 (u - u_old)) / dt phi_i phi_j + a(u) grad phi_i . grad phi_j
//                    + a1 phi_j (grad phi_i . grad u) ]
//
// k_nl_residual   one thread per element: u, u - u_old and grad u at every point from the rule tables and the
//                 device vectors (through the element dofs), the element vector written element-major
//                 (k_simplex_lf's E-vector; summed by k_e2l, then k_nl_finish: - g, essential rows zeroed);
// k_nl_gradient   one thread per element: the element matrix in k_simplex_elem's layout, so the gather, the
//                 eliminated matrix and the SELL copy of the full assembly run unchanged;
// k_bdr_lf        one thread per boundary facet: the facet's dofs from facet_dof's table over the element's local
//                 dof order, the facet E-vector summed per dof in ascending facet order (k_bdr_gather).
//                 (Quad / hex faces: k_bdr_lf_tensor of nl_fa_tensor.hip, the same gather.)
// No atomics: every sum has one fixed order.
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "point_geom.hpp"

namespace cdfem {

template <int DIM, int P>
constexpr int simplex_nd() { return P == 1 ? DIM + 1 : P == 2 ? (DIM + 1) * (DIM + 2) / 2 : 10; }

// u and u - u_old at the element's dofs; the difference is taken per dof, before the interpolation
template <int ND>
__device__ __forceinline__ void nl_gather(const int32_t *__restrict__ ed, const double *__restrict__ u,
                                          const double *__restrict__ uold, double (&ue)[ND], double (&de)[ND])
{
#pragma unroll
    for (int l = 0; l < ND; ++l) {
        const int32_t g = ed[l];
        ue[l] = u[g];
        de[l] = ue[l] - uold[g];
    }
}

// the state at one point: u, u - u_old, and t[b] = (W / det J) sum_k A[b][k] (sum_a A[a][k] d_a u), so that
// W det J (grad u . grad phi_i) = sum_b t[b] d_b phi_i.  The gradient is taken of u - u(vertex 0): the basis
// gradients sum to zero, so it is the same gradient, without the cancellation of u's constant part against the
// tables' rounding (a relative |u| / (h |grad u|) ulp of grad u: 1.6e4 ulp for the reference's u = 300)
template <int DIM, int ND>
__device__ __forceinline__ void nl_point(const double *__restrict__ phi, const double *__restrict__ dphi, double W,
                                         double det, const double (&A)[DIM][DIM], const double (&ue)[ND],
                                         const double (&de)[ND], double &uq, double &dq, double (&t)[DIM])
{
    double gr[DIM] = {};
    uq = 0.0;
    dq = 0.0;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        uq += phi[i] * ue[i];
        dq += phi[i] * de[i];
#pragma unroll
        for (int k = 0; k < DIM; ++k) gr[k] += dphi[i * DIM + k] * (ue[i] - ue[0]);
    }
    metric_flux<DIM>(A, W / det, gr, t);
}

template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_nl_residual(const double *__restrict__ verts, const int32_t *__restrict__ edofs, int ne, int nq,
              const double *__restrict__ tab, cdfem_nl_heat_coeffs k, const double *__restrict__ u,
              const double *__restrict__ uold, double *__restrict__ Ye)
{
    constexpr int ND = simplex_nd<DIM, P>();
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= ne) return;
    double A[DIM][DIM];
    const double det = simplex_adjugate<DIM>(verts + (size_t)e * (DIM + 1) * DIM, A);
    double ue[ND], de[ND], r[ND];
    nl_gather<ND>(edofs + (size_t)e * ND, u, uold, ue, de);
#pragma unroll
    for (int i = 0; i < ND; ++i) r[i] = 0.0;
    const double *phi_t = tab, *dphi_t = tab + (size_t)nq * ND, *w_t = tab + (size_t)nq * ND * (DIM + 1);
    const double idt = 1.0 / k.dt;
    for (int q = 0; q < nq; ++q) {
        const double *ph = phi_t + q * ND, *dph = dphi_t + (size_t)q * ND * DIM;
        double uq, dq, t[DIM];
        nl_point<DIM, ND>(ph, dph, w_t[q], det, A, ue, de, uq, dq, t);
        const double au = k.a0 + k.a1 * (uq - k.u_ref), mu = k.m0 + k.m1 * (uq - k.u_ref);
        const double cm = w_t[q] * det * mu * dq * idt;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            double v = ph[i] * cm;
#pragma unroll
            for (int b = 0; b < DIM; ++b) v += au * t[b] * dph[i * DIM + b];
            r[i] += v;
        }
    }
#pragma unroll
    for (int l = 0; l < ND; ++l) Ye[(size_t)e * ND + l] = r[l];
}

template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_nl_gradient(const double *__restrict__ verts, const int32_t *__restrict__ edofs, int ne, int nq,
              const double *__restrict__ tab, cdfem_nl_heat_coeffs k, const double *__restrict__ u,
              const double *__restrict__ uold, double *__restrict__ Ee)
{
    constexpr int ND = simplex_nd<DIM, P>();
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= ne) return;
    double A[DIM][DIM];
    const double det = simplex_adjugate<DIM>(verts + (size_t)e * (DIM + 1) * DIM, A);
    double ue[ND], de[ND];
    nl_gather<ND>(edofs + (size_t)e * ND, u, uold, ue, de);
    double M[ND][ND];
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) M[i][j] = 0.0;
    const double *phi_t = tab, *dphi_t = tab + (size_t)nq * ND, *w_t = tab + (size_t)nq * ND * (DIM + 1);
    const double idt = 1.0 / k.dt;
    for (int q = 0; q < nq; ++q) {
        const double W = w_t[q];
        double ph[ND], dph[ND][DIM];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            ph[i] = phi_t[q * ND + i];
#pragma unroll
            for (int a = 0; a < DIM; ++a) dph[i][a] = dphi_t[(q * ND + i) * DIM + a];
        }
        double uq, dq, t[DIM];
        nl_point<DIM, ND>(ph, &dph[0][0], W, det, A, ue, de, uq, dq, t);
        const double au = k.a0 + k.a1 * (uq - k.u_ref), mu = k.m0 + k.m1 * (uq - k.u_ref);
        const double Ms = W * det * (mu + k.m1 * dq) * idt;
        double D[DIM][DIM], Cv[DIM];
        const double f = W * au / det;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            Cv[a] = k.a1 * t[a];  // the transposed convection term, velocity a1 grad u
#pragma unroll
            for (int b = 0; b < DIM; ++b) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < DIM; ++m) s += A[a][m] * A[b][m];
                D[a][b] = f * s;
            }
        }
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            double Dg[DIM];
            const double rest = Ms * ph[j];
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                Dg[a] = Cv[a] * ph[j];
#pragma unroll
                for (int b = 0; b < DIM; ++b) Dg[a] += D[a][b] * dph[j][b];
            }
#pragma unroll
            for (int i = 0; i < ND; ++i) {
                double v = ph[i] * rest;
#pragma unroll
                for (int a = 0; a < DIM; ++a) v += dph[i][a] * Dg[a];
                M[i][j] += v;
            }
        }
    }
    const int64_t base = (int64_t)(e / kLanes) * ND * ND * kLanes + e % kLanes;
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) Ee[base + (int64_t)(i * ND + j) * kLanes] = M[i][j];
}

// R = R - g off the essential rows, 0 on them; negR (the Newton right-hand side) = -R
__global__ void __launch_bounds__(256)
k_nl_finish(const uint8_t *__restrict__ ess, const double *__restrict__ g, double *__restrict__ R,
            double *__restrict__ negR, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = ess[i] ? 0.0 : R[i] - g[i];
    R[i] = v;
    if (negR) negR[i] = -v;
}

// BoundaryLFIntegrator on facet t = (element, local facet f opposite vertex f): the facet's vertices are the
// element's other vertices in ascending local order, the measure factor the edge length (segment rule,
// weights summing to 1) or |t1 x t2| (triangle rule, weights summing to 1/2)
template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_bdr_lf(const double *__restrict__ verts, const int32_t *__restrict__ face_elem,
         const int32_t *__restrict__ face_local, int nbf, int nqb, const double *__restrict__ btab,
         const double *__restrict__ gq, double *__restrict__ Ye)
{
    constexpr int NF = facet_ndofs(DIM, P);
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nbf) return;
    const int f = face_local[t];
    const double *V = verts + (size_t)face_elem[t] * (DIM + 1) * DIM;
    int v[DIM];
    for (int a = 0, m = 0; a <= DIM; ++a)
        if (a != f) v[m++] = a;
    double meas;
    if constexpr (DIM == 2) {
        const double dx = V[v[1] * 2] - V[v[0] * 2], dy = V[v[1] * 2 + 1] - V[v[0] * 2 + 1];
        meas = sqrt(dx * dx + dy * dy);
    } else {
        double t1[3], t2[3];
        for (int k = 0; k < 3; ++k) {
            t1[k] = V[v[1] * 3 + k] - V[v[0] * 3 + k];
            t2[k] = V[v[2] * 3 + k] - V[v[0] * 3 + k];
        }
        const double cx = t1[1] * t2[2] - t1[2] * t2[1], cy = t1[2] * t2[0] - t1[0] * t2[2],
                     cz = t1[0] * t2[1] - t1[1] * t2[0];
        meas = sqrt(cx * cx + cy * cy + cz * cz);
    }
    double b[NF];
#pragma unroll
    for (int l = 0; l < NF; ++l) b[l] = 0.0;
    const double *w_t = btab + (size_t)(DIM + 1) * nqb * NF;
    for (int q = 0; q < nqb; ++q) {
        const double fw = w_t[q] * meas * gq[(size_t)t * nqb + q];
        const double *ph = btab + ((size_t)f * nqb + q) * NF;
#pragma unroll
        for (int l = 0; l < NF; ++l) b[l] += fw * ph[l];
    }
#pragma unroll
    for (int l = 0; l < NF; ++l) Ye[(size_t)t * NF + l] = b[l];
}

__global__ void __launch_bounds__(256)
k_bdr_gather(const int32_t *__restrict__ off, const int32_t *__restrict__ pos, const double *__restrict__ Ye,
             double *__restrict__ b, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    for (int32_t k = off[i]; k < off[i + 1]; ++k) v += Ye[pos[k]];
    b[i] = v;
}

// ---- launchers ---------------------------------------------------------------------------------
hipError_t launch_nl_residual(cdfem_ctx *c, const double *u, double *Ye)
{
    const dim3 g((c->ne + 63) / 64), b(64);
    return dispatch_simplex(c, [&](auto D, auto P) {
        hipLaunchKernelGGL((k_nl_residual<D(), P()>), g, b, 0, c->stream, c->d_verts.get(), c->heat.d_edofs.get(), c->ne,
                           c->heat.nq, c->heat.d_tab.get(), nl_coeffs(c), u, c->heat.d_uold.get(), Ye);
        return hipGetLastError();
    });
}

hipError_t launch_nl_gradient(cdfem_ctx *c, const double *u)
{
    const dim3 g((c->ne + 63) / 64), b(64);
    return dispatch_simplex(c, [&](auto D, auto P) {
        hipLaunchKernelGGL((k_nl_gradient<D(), P()>), g, b, 0, c->stream, c->d_verts.get(), c->heat.d_edofs.get(), c->ne,
                           c->heat.nq, c->heat.d_tab.get(), nl_coeffs(c), u, c->heat.d_uold.get(), c->d_Ee.get());
        return hipGetLastError();
    });
}

hipError_t launch_nl_finish(cdfem_ctx *c, double *R, const double *g, double *negR)
{
    hipLaunchKernelGGL(k_nl_finish, dim3((unsigned)((c->nl + 255) / 256)), dim3(256), 0, c->stream, c->d_ess.get(), g, R,
                       negR, (int64_t)c->nl);
    return hipGetLastError();
}

hipError_t launch_bdr_lf(cdfem_ctx *c, const double *gq, double *b)
{
    if (c->heat.nbf > 0) {
        const dim3 g((c->heat.nbf + 63) / 64), blk(64);
        const hipError_t e = c->geom == 0 ? launch_bdr_lf_tensor(c, gq) : dispatch_simplex(c, [&](auto D, auto P) {
            hipLaunchKernelGGL((k_bdr_lf<D(), P()>), g, blk, 0, c->stream, c->d_verts.get(), c->heat.d_face_elem.get(),
                               c->heat.d_face_local.get(), c->heat.nbf, c->heat.nqb, c->heat.d_btab.get(), gq,
                               c->heat.d_bYe.get());
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bdr_gather, dim3((unsigned)((c->nl + 255) / 256)), dim3(256), 0, c->stream,
                       c->heat.d_b_off.get(), c->heat.d_b_pos.get(), c->heat.d_bYe.get(), b, (int64_t)c->nl);
    return hipGetLastError();
}

}  // namespace cdfem
