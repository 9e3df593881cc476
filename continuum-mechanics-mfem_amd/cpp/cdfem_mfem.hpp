// cdfem_mfem.hpp — MFEM-shaped C++ host API over the cdfem C-ABI (include/cdfem.h).
//
// The host side of the drop-in boundary: the classes and member functions the
// reference drivers call on their hot path, with MFEM's names, argument meaning, ownership rules and
// MPI semantics, backed by the MI355X kernels.  `cpp/mfem.hpp` makes `#include "mfem.hpp"` +
// `using namespace mfem;` resolve to this header.
//
//   reference call (linear_convection_diffusion_2D.cpp unless stated)   here
//   Mpi::Init / Hypre::Init / Mpi::WorldRank (:240-242)                  Mpi, Hypre (MPI_Init, MPICH)
//   OptionsParser (:245-253)                                             OptionsParser
//   Device device("cpu"); device.Print() (:287-288)                      Device (one MI355X per rank)
//   Mesh(file, 1, 1), UniformRefinement, MakeCartesian* (:290-298)       Mesh (gmsh v2.2 simplices / boxes)
//   ParMesh(MPI_COMM_WORLD, *mesh), GetNV/GetVertex (:300-309,136-138)   ParMesh: z-slabs of a box, else an
//                                                                        RCB element partition
//   H1_FECollection, ParFiniteElementSpace, GlobalTrueVSize (:311-317)   FiniteElementSpace (local L-dofs,
//                                                                        true dofs = the owned suffix)
//   GetEssentialTrueDofs(ess_bdr, list) (:319-322)                       true-dof list, as MFEM
//   Coefficient::Eval(T, ip), T.Transform(ip, x) (:159-215)              Coefficient, ElementTransformation
//   MatrixCoefficient (diffusion_mms_ale.cpp:474-502)                    MatrixCoefficient, DenseMatrix
//   ParBilinearForm + Diffusion/Convection/MassIntegrator (:335-339)     BilinearForm (PA on hexes/quads,
//                                                                        FA on simplices; owns integrators)
//   ParLinearForm + DomainLFIntegrator (:341-343)                        LinearForm (rank-local partial)
//   ParGridFunction::ProjectBdrCoefficient (:345-347)                    GridFunction (L-vector)
//   FormLinearSystem(ess, u, b, A, X, B) (:349-351)                      X, B true-dof vectors (P^T b)
//   Ah.As<HypreParMatrix>() (:364)                                       the constrained operator
//   PetscParMatrix(MPI_COMM_WORLD, A, PETSC_MATAIJ) (:367),              PetscParMatrix, PetscLinearSolver
//   PetscParMatrix(A_hyp, PETSC_MATAIJ) (diffusion_mms.cpp:449),           (GPU GMRES / CG; option keys of
//   PetscLinearSolver + options file (:268-282,368-374)                   Input/petsc.opts, with prefixes)
//   MFEM_VERIFY (:150,307,365,371)                                       MFEM_VERIFY (throws)
//   RecoverFEMSolution (:377)                                            x = P X
//   ComputeL2Error / ComputeGlobalLpNorm (:383-392)                      MPI-reduced over the ranks
//   ComputeLpError(2, exact, &weight, irs) (diffusion_mms_ale.cpp:924)   weighted L2
//
// Error behaviour: every failing C-ABI call throws std::runtime_error carrying cdfem_last_error (the
// reference drivers catch std::exception at main and return 3, :435-442); MFEM_VERIFY throws
// std::runtime_error; size misuse throws std::invalid_argument.  There is no CPU fallback:
// constructing a form without a GPU throws.
//
// Parallel model (MFEM's): one rank per GPU.  A GridFunction / LinearForm / BilinearForm::Mult
// vector is a rank-local L-vector (shared dofs duplicated; a LinearForm or a local Mult holds
// partial sums).  FormLinearSystem returns true-dof vectors X, B (the dofs this rank owns: the lowest
// rank holding a shared dof owns it) and the constrained operator P^T A P on them; RecoverFEMSolution
// is x = P X.  The ranks exchange through RCCL when every rank has its own GPU, otherwise through MPI
// (CDFEM_COMM=rccl|host overrides).  -pc_type bjacobi on several ranks: one ILU(0) block per rank.
#pragma once

#include <mpi.h>

#include <algorithm>
#include <array>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "cdfem.h"

// MFEM_VERIFY(condition, message-stream) as in MFEM with exceptions enabled: the message may use
// operator<< (linear_convection_diffusion_2D.cpp:150-156, :371-374)
#define MFEM_VERIFY(x, msg)                                                                        \
    do {                                                                                           \
        if (!(x)) {                                                                                \
            std::ostringstream mfem_verify_msg_;                                                   \
            mfem_verify_msg_ << "Verification failed: (" << #x << ") is false:\n --> " << msg;    \
            throw std::runtime_error(mfem_verify_msg_.str());                                      \
        }                                                                                          \
    } while (0)
#define MFEM_ABORT(msg)                                                                            \
    do {                                                                                           \
        std::ostringstream mfem_abort_msg_;                                                        \
        mfem_abort_msg_ << msg;                                                                    \
        throw std::runtime_error(mfem_abort_msg_.str());                                           \
    } while (0)

namespace cdfem {
namespace mfem {

using real_t = double;
using HYPRE_BigInt = long long;

inline void check(int rc, const cdfem_ctx *ctx, const char *what)
{
    if (rc == CDFEM_OK) return;
    std::string msg = std::string(what) + " failed (status " + std::to_string(rc) + ")";
    if (ctx) msg += ": " + std::string(cdfem_last_error(ctx));
    throw std::runtime_error(msg);
}

// ---- MPI, hypre and device set-up ------------------------------------------------------------
class Mpi {
public:
    static bool IsInitialized()
    {
        int f = 0;
        MPI_Initialized(&f);
        return f != 0;
    }
    static void Init(int &argc, char **&argv)
    {
        if (IsInitialized()) return;
        MPI_Init(&argc, &argv);
        std::atexit(Finalize);
    }
    static void Init()
    {
        if (IsInitialized()) return;
        MPI_Init(nullptr, nullptr);
        std::atexit(Finalize);
    }
    static void Finalize()
    {
        int fin = 0;
        MPI_Finalized(&fin);
        if (IsInitialized() && !fin) MPI_Finalize();
    }
    static int WorldRank()
    {
        int r = 0;
        if (IsInitialized()) MPI_Comm_rank(MPI_COMM_WORLD, &r);
        return r;
    }
    static int WorldSize()
    {
        int n = 1;
        if (IsInitialized()) MPI_Comm_size(MPI_COMM_WORLD, &n);
        return n;
    }
    static bool Root() { return WorldRank() == 0; }
};

class Hypre {
public:
    static void Init() {}  // hypre is not used: the assembled and matrix-free operators are the library's
};

namespace detail {

inline int comm_rank(MPI_Comm c)
{
    int r = 0;
    if (Mpi::IsInitialized()) MPI_Comm_rank(c, &r);
    return r;
}
inline int comm_size(MPI_Comm c)
{
    int n = 1;
    if (Mpi::IsInitialized()) MPI_Comm_size(c, &n);
    return n;
}

// ranks on this node (MPI_COMM_TYPE_SHARED) and this rank's index among them
inline void node_rank_size(int &r, int &n)
{
    r = 0;
    n = 1;
    if (!Mpi::IsInitialized()) return;
    MPI_Comm node;
    MPI_Comm_split_type(MPI_COMM_WORLD, MPI_COMM_TYPE_SHARED, 0, MPI_INFO_NULL, &node);
    MPI_Comm_rank(node, &r);
    MPI_Comm_size(node, &n);
    MPI_Comm_free(&node);
}

// host-communicator callbacks over MPI (the user pointer is the MPI_Comm)
inline int mpi_allreduce(double *buf, int n, void *user)
{
    return MPI_Allreduce(MPI_IN_PLACE, buf, n, MPI_DOUBLE, MPI_SUM, *static_cast<MPI_Comm *>(user)) == MPI_SUCCESS ? 0 : 1;
}
inline int mpi_plane_exchange(const double *slo, double *rlo, const double *shi, double *rhi, int64_t n, void *user)
{
    const MPI_Comm c = *static_cast<MPI_Comm *>(user);
    const int r = comm_rank(c);
    MPI_Request req[4];
    int k = 0;
    if (slo) {
        MPI_Isend(slo, (int)n, MPI_DOUBLE, r - 1, 71, c, &req[k++]);
        MPI_Irecv(rlo, (int)n, MPI_DOUBLE, r - 1, 72, c, &req[k++]);
    }
    if (shi) {
        MPI_Isend(shi, (int)n, MPI_DOUBLE, r + 1, 72, c, &req[k++]);
        MPI_Irecv(rhi, (int)n, MPI_DOUBLE, r + 1, 71, c, &req[k++]);
    }
    return MPI_Waitall(k, req, MPI_STATUSES_IGNORE) == MPI_SUCCESS ? 0 : 1;
}
inline int mpi_nbr_exchange(int nn, const int32_t *ranks, const int64_t *off, const double *send, double *recv, void *user)
{
    const MPI_Comm c = *static_cast<MPI_Comm *>(user);
    std::vector<MPI_Request> req(2 * (size_t)nn);
    for (int k = 0; k < nn; ++k) {
        const int cnt = (int)(off[k + 1] - off[k]);
        MPI_Isend(send + off[k], cnt, MPI_DOUBLE, ranks[k], 73, c, &req[2 * k]);
        MPI_Irecv(recv + off[k], cnt, MPI_DOUBLE, ranks[k], 73, c, &req[2 * k + 1]);
    }
    return MPI_Waitall(2 * nn, req.data(), MPI_STATUSES_IGNORE) == MPI_SUCCESS ? 0 : 1;
}

// process-wide state: the device of this rank and the communicator every context shares
struct Runtime {
    int device = -1;
    std::string requested = "cpu";
    cdfem_ctx *anchor = nullptr;  // context that owns the rank communicator (cdfem_comm_share)
    MPI_Comm comm = MPI_COMM_WORLD;
    std::string backend = "none";
    ~Runtime()
    {
        if (anchor) cdfem_destroy(anchor);
    }
};
inline Runtime &runtime()
{
    static Runtime rt;
    return rt;
}

inline int device_id()
{
    Runtime &rt = runtime();
    if (rt.device >= 0) return rt.device;
    if (const char *d = std::getenv("CDFEM_DEVICE")) return rt.device = std::atoi(d);
    const int ndev = cdfem_device_count();
    int r = 0, n = 1;
    node_rank_size(r, n);
    rt.device = ndev > 0 ? r % ndev : 0;
    return rt.device;
}

// the communicator of MPI_COMM_WORLD, created once on first use by a partitioned space
inline cdfem_ctx *comm_anchor()
{
    Runtime &rt = runtime();
    if (rt.anchor) return rt.anchor;
    const int size = comm_size(rt.comm), rank = comm_rank(rt.comm);
    cdfem_ctx *a = nullptr;
    check(cdfem_create(device_id(), &a), nullptr, "cdfem_create (no GPU? there is no CPU path)");
    int nr = 0, nn = 1;
    node_rank_size(nr, nn);
    const char *force = std::getenv("CDFEM_COMM");
    const bool rccl = force ? std::string(force) == "rccl" : nn <= cdfem_device_count();
    if (rccl) {
        unsigned char id[128] = {};
        if (rank == 0) check(cdfem_comm_unique_id(id), nullptr, "cdfem_comm_unique_id");
        MPI_Bcast(id, 128, MPI_UNSIGNED_CHAR, 0, rt.comm);
        check(cdfem_comm_init_rccl(a, rank, size, id), a, "cdfem_comm_init_rccl");
        rt.backend = "rccl";
    } else {
        check(cdfem_comm_init_host(a, rank, size, mpi_allreduce, mpi_plane_exchange, &rt.comm), a,
              "cdfem_comm_init_host");
        check(cdfem_comm_set_host_nbr_exchange(a, mpi_nbr_exchange, &rt.comm), a, "cdfem_comm_set_host_nbr_exchange");
        rt.backend = "host (MPI)";
    }
    rt.anchor = a;
    return a;
}

inline double allreduce_sum(double v, MPI_Comm c)
{
    if (!Mpi::IsInitialized() || comm_size(c) == 1) return v;
    double out = 0.0;
    MPI_Allreduce(&v, &out, 1, MPI_DOUBLE, MPI_SUM, c);
    return out;
}

}  // namespace detail

// Device("cpu") in the reference selects MFEM's CPU backend; here every rank's forms run on one
// MI355X (the local rank's GPU), whatever the string says (there is no CPU path).
class Device {
public:
    explicit Device(const std::string &spec = "cpu")
    {
        detail::runtime().requested = spec;
        (void)detail::device_id();
    }
    void Print(std::ostream &os = std::cout) const
    {
        os << "Device configuration: requested '" << detail::runtime().requested << "', running on HIP device "
           << detail::device_id() << " (MI355X, gfx950) of " << cdfem_device_count() << " visible\n";
    }
};

// ---- containers ---------------------------------------------------------------------------------
namespace detail {
// Device memory behind Vectors: one allocation/copy context per process, a free list per size (the
// reference's time loop builds a ParLinearForm, a PetscParMatrix and a solver every step,
// diffusion_mms.cpp:428-456), never handed back (process lifetime).  CDFEM_SHIM_STATS=1 prints the
// host<->device traffic of the Vectors at exit (tests/test_cpp_driver.py counts it per time step).
struct DeviceMemory {
    cdfem_ctx *ctx = nullptr;
    std::map<size_t, std::vector<double *>> free_;
    unsigned long long h2d = 0, d2h = 0, h2d_calls = 0, d2h_calls = 0;
};
inline void print_shim_stats();
inline DeviceMemory &devmem()
{
    static DeviceMemory *m = [] {
        auto *d = new DeviceMemory();  // leaked on purpose: Vectors may outlive every static
        if (const char *e = std::getenv("CDFEM_SHIM_STATS"); e && *e && *e != '0') std::atexit(print_shim_stats);
        return d;
    }();
    return *m;
}
inline void print_shim_stats()
{
    const DeviceMemory &m = devmem();
    std::fprintf(stderr, "shim_transfers rank %d h2d_bytes %llu h2d_calls %llu d2h_bytes %llu d2h_calls %llu\n",
                 Mpi::WorldRank(), m.h2d, m.h2d_calls, m.d2h, m.d2h_calls);
}
inline cdfem_ctx *mem_ctx()
{
    DeviceMemory &m = devmem();
    if (!m.ctx) check(cdfem_create(device_id(), &m.ctx), nullptr, "cdfem_create (no GPU? there is no CPU path)");
    return m.ctx;
}
inline double *dev_alloc(size_t n)
{
    DeviceMemory &m = devmem();
    auto it = m.free_.find(n);
    if (it != m.free_.end() && !it->second.empty()) {
        double *p = it->second.back();
        it->second.pop_back();
        return p;
    }
    void *p = nullptr;
    check(cdfem_alloc(mem_ctx(), n * sizeof(double), &p), mem_ctx(), "cdfem_alloc");
    return static_cast<double *>(p);
}
inline void dev_release(double *p, size_t n)
{
    if (p) devmem().free_[n].push_back(p);
}
inline void dev_copy(void *dst, int dw, const void *src, int sw, size_t n)
{
    if (n == 0) return;
    DeviceMemory &m = devmem();
    if (dw == CDFEM_DEVICE && sw == CDFEM_HOST) m.h2d += n * sizeof(double), ++m.h2d_calls;
    if (dw == CDFEM_HOST && sw == CDFEM_DEVICE) m.d2h += n * sizeof(double), ++m.d2h_calls;
    check(cdfem_memcpy(mem_ctx(), dst, dw, src, sw, n * sizeof(double)), mem_ctx(), "cdfem_memcpy");
}
}  // namespace detail

// MFEM's Vector with its Memory<double> semantics (UseDevice): a host array and a device copy with
// validity flags.  Host access (GetData, operator[], HostRead / HostWrite / HostReadWrite) copies the
// device data back when only the device copy is current; the forms, FormLinearSystem, the solvers
// and RecoverFEMSolution work on the device copy (Read / Write / ReadWrite), so a time loop's vectors
// stay in HBM between those calls and cross PCIe only where the host touches them (coefficient
// projection, error norms).
class Vector {
public:
    Vector() = default;
    explicit Vector(int n) : d_((size_t)n, 0.0) {}
    Vector(const double *p, int n) : d_(p, p + n) {}
    Vector(const Vector &o) { assign(o); }
    Vector(Vector &&o) noexcept { steal(o); }
    Vector &operator=(const Vector &o)
    {
        if (this != &o) assign(o);
        return *this;
    }
    Vector &operator=(Vector &&o) noexcept
    {
        if (this != &o) {
            detail::dev_release(dev_, d_.size());
            steal(o);
        }
        return *this;
    }
    virtual ~Vector() { detail::dev_release(dev_, d_.size()); }
    int Size() const { return (int)d_.size(); }
    void SetSize(int n)
    {
        if ((size_t)n == d_.size()) return;
        sync_host();
        detail::dev_release(dev_, d_.size());
        dev_ = nullptr;
        dev_ok_ = false;
        d_.resize((size_t)n, 0.0);
    }
    // host access
    const double *HostRead() const
    {
        sync_host();
        return d_.data();
    }
    double *HostReadWrite()
    {
        sync_host();
        dev_ok_ = false;
        return d_.data();
    }
    double *HostWrite()
    {
        host_ok_ = true;
        dev_ok_ = false;
        return d_.data();
    }
    // device access (HBM pointers for the C-ABI's CDFEM_DEVICE calls)
    const double *Read() const
    {
        if (!dev_) dev_ = detail::dev_alloc(d_.size());
        if (!dev_ok_) {
            detail::dev_copy(dev_, CDFEM_DEVICE, d_.data(), CDFEM_HOST, d_.size());
            dev_ok_ = true;
        }
        return dev_;
    }
    double *Write()
    {
        if (!dev_) dev_ = detail::dev_alloc(d_.size());
        dev_ok_ = true;
        host_ok_ = false;
        return dev_;
    }
    double *ReadWrite()
    {
        Read();
        host_ok_ = false;
        return dev_;
    }
    bool DeviceIsValid() const { return dev_ok_; }
    bool HostIsValid() const { return host_ok_; }

    double *GetData() { return HostReadWrite(); }
    const double *GetData() const { return HostRead(); }
    double &operator[](int i) { return HostReadWrite()[(size_t)i]; }
    double operator[](int i) const { return HostRead()[(size_t)i]; }
    double &operator()(int i) { return HostReadWrite()[(size_t)i]; }
    double operator()(int i) const { return HostRead()[(size_t)i]; }
    Vector &operator=(double v)
    {
        std::fill(d_.begin(), d_.end(), v);
        HostWrite();
        return *this;
    }
    Vector &operator*=(double a)
    {
        for (double *p = HostReadWrite(), *e = p + d_.size(); p != e; ++p) *p *= a;
        return *this;
    }
    Vector &operator+=(const Vector &o)
    {
        const double *q = o.HostRead();
        double *p = HostReadWrite();
        for (size_t i = 0; i < d_.size(); ++i) p[i] += q[i];
        return *this;
    }
    Vector &operator-=(const Vector &o)
    {
        const double *q = o.HostRead();
        double *p = HostReadWrite();
        for (size_t i = 0; i < d_.size(); ++i) p[i] -= q[i];
        return *this;
    }
    double operator*(const Vector &o) const
    {
        const double *p = HostRead(), *q = o.HostRead();
        double s = 0.0;
        for (size_t i = 0; i < d_.size(); ++i) s += p[i] * q[i];
        return s;
    }
    double Norml2() const { return std::sqrt((*this) * (*this)); }
    double Normlinf() const
    {
        const double *p = HostRead();
        double m = 0.0;
        for (size_t i = 0; i < d_.size(); ++i) m = std::max(m, std::fabs(p[i]));
        return m;
    }
    double Sum() const
    {
        const double *p = HostRead();
        return std::accumulate(p, p + d_.size(), 0.0);
    }
    // this += a x: on the device when both device copies are current and one side has no current
    // host copy (rhs.Add(dt, f) of diffusion_mms.cpp:433: M u_old and the linear form, both fresh
    // from the GPU), else on the host
    void Add(double a, const Vector &x)
    {
        if (x.Size() != Size()) throw std::invalid_argument("Vector::Add: size");
        if (dev_ok_ && x.dev_ok_ && !(host_ok_ && x.host_ok_) && !d_.empty()) {
            check(cdfem_vec_axpby(detail::mem_ctx(), (int64_t)d_.size(), a, x.Read(), 1.0, ReadWrite()),
                  detail::mem_ctx(), "cdfem_vec_axpby");
            return;
        }
        const double *q = x.HostRead();
        double *p = HostReadWrite();
        for (size_t i = 0; i < d_.size(); ++i) p[i] += a * q[i];
    }
    void Neg()
    {
        for (double *p = HostReadWrite(), *e = p + d_.size(); p != e; ++p) *p = -*p;
    }
    // this = src[off, off + n) without a host round trip when src lives on the device
    void SetSubVectorOf(const Vector &src, int off, int n)
    {
        if (off < 0 || n < 0 || off + n > src.Size()) throw std::invalid_argument("SetSubVectorOf: range");
        SetSize(n);
        if (src.dev_ok_ && !src.host_ok_) {
            if (n) detail::dev_copy(Write(), CDFEM_DEVICE, src.dev_ + off, CDFEM_DEVICE, (size_t)n);
            else Write();
            return;
        }
        const double *q = src.HostRead() + off;
        std::copy(q, q + n, HostWrite());
    }

private:
    void sync_host() const
    {
        if (host_ok_) return;
        detail::dev_copy(d_.data(), CDFEM_HOST, dev_, CDFEM_DEVICE, d_.size());
        host_ok_ = true;
    }
    void assign(const Vector &o)
    {
        if (o.d_.size() != d_.size()) {
            detail::dev_release(dev_, d_.size());
            dev_ = nullptr;
            d_.assign(o.d_.size(), 0.0);
        }
        if (o.dev_ok_ && !o.host_ok_) {  // device-only source: copy in HBM
            if (!d_.empty()) detail::dev_copy(Write(), CDFEM_DEVICE, o.dev_, CDFEM_DEVICE, d_.size());
            else Write();
            return;
        }
        std::copy(o.d_.begin(), o.d_.end(), d_.begin());
        HostWrite();
    }
    void steal(Vector &o)
    {
        d_ = std::move(o.d_);
        dev_ = o.dev_;
        host_ok_ = o.host_ok_;
        dev_ok_ = o.dev_ok_;
        o.d_.clear();
        o.dev_ = nullptr;
        o.host_ok_ = true;
        o.dev_ok_ = false;
    }
    mutable std::vector<double> d_;  // mutable: a const read refreshes the host copy
    mutable double *dev_ = nullptr;
    mutable bool host_ok_ = true, dev_ok_ = false;
};

inline void subtract(const Vector &a, const Vector &b, Vector &c)
{
    c.SetSize(a.Size());
    const double *p = a.HostRead(), *q = b.HostRead();
    double *r = c.HostWrite();
    for (int i = 0; i < a.Size(); ++i) r[i] = p[i] - q[i];
}

template <class T>
class Array {
public:
    Array() = default;
    explicit Array(int n) : d_((size_t)n) {}
    int Size() const { return (int)d_.size(); }
    void SetSize(int n) { d_.resize((size_t)n); }
    void Append(const T &v) { d_.push_back(v); }
    T &operator[](int i) { return d_[(size_t)i]; }
    const T &operator[](int i) const { return d_[(size_t)i]; }
    Array &operator=(const T &v)
    {
        std::fill(d_.begin(), d_.end(), v);
        return *this;
    }
    T Max() const { return d_.empty() ? T() : *std::max_element(d_.begin(), d_.end()); }
    T *GetData() { return d_.data(); }
    const T *GetData() const { return d_.data(); }
    bool operator==(const Array &o) const { return d_ == o.d_; }

private:
    std::vector<T> d_;
};

class DenseMatrix {
public:
    DenseMatrix() = default;
    explicit DenseMatrix(int n) : DenseMatrix(n, n) {}
    DenseMatrix(int h, int w) : h_(h), w_(w), d_((size_t)h * w, 0.0) {}
    void SetSize(int n) { SetSize(n, n); }
    void SetSize(int h, int w)
    {
        h_ = h;
        w_ = w;
        d_.assign((size_t)h * w, 0.0);
    }
    int Height() const { return h_; }
    int Width() const { return w_; }
    double &operator()(int i, int j) { return d_[(size_t)j * h_ + i]; }  // column-major, as MFEM
    double operator()(int i, int j) const { return d_[(size_t)j * h_ + i]; }
    DenseMatrix &operator=(double v)
    {
        std::fill(d_.begin(), d_.end(), v);
        return *this;
    }
    DenseMatrix &operator*=(double a)
    {
        for (double &v : d_) v *= a;
        return *this;
    }

private:
    int h_ = 0, w_ = 0;
    std::vector<double> d_;
};

// AAt = A A^T (MFEM MultAAt, used by the ALE metric, diffusion_mms_ale.cpp:494)
inline void MultAAt(const DenseMatrix &A, DenseMatrix &AAt)
{
    AAt.SetSize(A.Height(), A.Height());
    for (int i = 0; i < A.Height(); ++i)
        for (int j = 0; j < A.Height(); ++j) {
            double s = 0.0;
            for (int k = 0; k < A.Width(); ++k) s += A(i, k) * A(j, k);
            AAt(i, j) = s;
        }
}

// ---- geometry / quadrature -----------------------------------------------------------------------
struct IntegrationPoint {
    double x = 0.0, y = 0.0, z = 0.0, weight = 0.0;
};

struct Geometry {
    enum Type { INVALID = -1, POINT = 0, SEGMENT, TRIANGLE, SQUARE, TETRAHEDRON, CUBE, PRISM, PYRAMID, NUM_GEOMETRIES };
    static constexpr int NumGeom = NUM_GEOMETRIES;
};

// A rule identified by geometry and polynomial order (IntRules.Get); the error functionals use
// Gauss-Legendre with n = order / 2 + 1 points per direction on tensor elements.
class IntegrationRule {
public:
    IntegrationRule() = default;
    IntegrationRule(int geom, int order) : geom_(geom), order_(order) {}
    int GetOrder() const { return order_; }
    int GetGeometry() const { return geom_; }

private:
    int geom_ = Geometry::SQUARE, order_ = 2;
};

class IntegrationRules {
public:
    const IntegrationRule &Get(int geom, int order)
    {
        const int key = geom * 1024 + order;
        auto it = rules_.find(key);
        if (it == rules_.end()) it = rules_.emplace(key, IntegrationRule(geom, order)).first;
        return it->second;
    }

private:
    std::map<int, IntegrationRule> rules_;
};
inline IntegrationRules IntRules;

// The physical point of the quadrature point being sampled; user coefficients call
// T.Transform(ip, x) exactly as in the reference (linear_convection_diffusion_2D.cpp:166-168).
class ElementTransformation {
public:
    int ElementNo = -1;
    int Attribute = 1;
    // a point transformation (the library evaluates coefficients at physical points: X is fixed),
    // or an affine boundary element X0 + xi E0 + eta E1 (Mesh::GetBdrElementTransformation)
    void Transform(const IntegrationPoint &ip, Vector &x) const
    {
        x.SetSize(dim_);
        for (int k = 0; k < dim_; ++k) x[k] = X_[k] + ip.x * E_[0][k] + ip.y * E_[1][k];
    }
    void SetPoint(int dim, const double *X)
    {
        dim_ = dim;
        geom_ = Geometry::POINT;
        for (int k = 0; k < dim; ++k) {
            X_[k] = X[k];
            E_[0][k] = E_[1][k] = 0.0;
        }
    }
    void SetAffine(int dim, Geometry::Type geom, const double *X0, const double *E0, const double *E1)
    {
        dim_ = dim;
        geom_ = geom;
        for (int k = 0; k < dim; ++k) {
            X_[k] = X0[k];
            E_[0][k] = E0 ? E0[k] : 0.0;
            E_[1][k] = E1 ? E1[k] : 0.0;
        }
    }
    Geometry::Type GetGeometryType() const { return geom_; }

private:
    int dim_ = 0;
    Geometry::Type geom_ = Geometry::POINT;
    double X_[3] = {0, 0, 0};
    double E_[2][3] = {{0, 0, 0}, {0, 0, 0}};
};

// MFEM's Geometries (reference-element data): GetCenter, as BuildXDirichletBoundaryMarker uses it
// (linear_convection_diffusion_1D.cpp:242)
struct GeometryRefs {
    const IntegrationPoint &GetCenter(int geom) const
    {
        static const IntegrationPoint c[Geometry::NumGeom] = {
            {0.0, 0.0, 0.0, 1.0},                       // POINT
            {0.5, 0.0, 0.0, 1.0},                       // SEGMENT
            {1.0 / 3.0, 1.0 / 3.0, 0.0, 0.5},           // TRIANGLE
            {0.5, 0.5, 0.0, 1.0},                       // SQUARE
            {0.25, 0.25, 0.25, 1.0 / 6.0},              // TETRAHEDRON
            {0.5, 0.5, 0.5, 1.0},                       // CUBE
            {1.0 / 3.0, 1.0 / 3.0, 0.5, 0.5},           // PRISM
            {0.4, 0.4, 0.2, 1.0 / 3.0}};                // PYRAMID
        if (geom < 0 || geom >= Geometry::NumGeom) throw std::invalid_argument("GetCenter: geometry");
        return c[geom];
    }
};
inline const GeometryRefs Geometries{};

// ---- coefficients --------------------------------------------------------------------------------
class Coefficient {
public:
    virtual ~Coefficient() = default;
    virtual real_t Eval(ElementTransformation &T, const IntegrationPoint &ip) = 0;
    virtual void SetTime(double t) { time = t; }
    double GetTime() const { return time; }

protected:
    double time = 0.0;
};

class ConstantCoefficient : public Coefficient {
public:
    double constant;
    explicit ConstantCoefficient(double c = 1.0) : constant(c) {}
    real_t Eval(ElementTransformation &, const IntegrationPoint &) override { return constant; }
};

class FunctionCoefficient : public Coefficient {
public:
    explicit FunctionCoefficient(std::function<double(const Vector &)> f) : f_(std::move(f)) {}
    explicit FunctionCoefficient(std::function<double(const Vector &, double)> ft) : ft_(std::move(ft)) {}
    real_t Eval(ElementTransformation &T, const IntegrationPoint &ip) override
    {
        Vector x;
        T.Transform(ip, x);
        return f_ ? f_(x) : ft_(x, time);
    }

private:
    std::function<double(const Vector &)> f_;
    std::function<double(const Vector &, double)> ft_;
};

class ProductCoefficient : public Coefficient {
public:
    ProductCoefficient(double a, Coefficient &b) : a_(a), b_(&b) {}
    ProductCoefficient(Coefficient &a, Coefficient &b) : ac_(&a), b_(&b) {}
    real_t Eval(ElementTransformation &T, const IntegrationPoint &ip) override
    {
        return (ac_ ? ac_->Eval(T, ip) : a_) * b_->Eval(T, ip);
    }

private:
    double a_ = 1.0;
    Coefficient *ac_ = nullptr, *b_;
};

class VectorCoefficient {
public:
    explicit VectorCoefficient(int vd) : vdim(vd) {}
    virtual ~VectorCoefficient() = default;
    int GetVDim() const { return vdim; }
    virtual void Eval(Vector &V, ElementTransformation &T, const IntegrationPoint &ip) = 0;
    virtual void SetTime(double t) { time = t; }
    double GetTime() const { return time; }

protected:
    int vdim;
    double time = 0.0;
};

class VectorConstantCoefficient : public VectorCoefficient {
public:
    explicit VectorConstantCoefficient(const Vector &v) : VectorCoefficient(v.Size()), vec(v) {}
    void Eval(Vector &V, ElementTransformation &, const IntegrationPoint &) override { V = vec; }
    const Vector &GetVec() const { return vec; }

private:
    Vector vec;
};

class VectorFunctionCoefficient : public VectorCoefficient {
public:
    VectorFunctionCoefficient(int dim, std::function<void(const Vector &, Vector &)> f)
        : VectorCoefficient(dim), f_(std::move(f)) {}
    void Eval(Vector &V, ElementTransformation &T, const IntegrationPoint &ip) override
    {
        Vector x;
        T.Transform(ip, x);
        V.SetSize(vdim);
        f_(x, V);
    }

private:
    std::function<void(const Vector &, Vector &)> f_;
};

// DiffusionIntegrator(MatrixCoefficient&): a symmetric tensor per quadrature point (the ALE metric,
// diffusion_mms_ale.cpp:474-502); a non-symmetric value is rejected at assembly.
class MatrixCoefficient {
public:
    explicit MatrixCoefficient(int dim, bool symm = false) : height(dim), width(dim), symmetric(symm) {}
    virtual ~MatrixCoefficient() = default;
    int GetHeight() const { return height; }
    int GetWidth() const { return width; }
    int GetVDim() const { return width; }
    bool IsSymmetric() const { return symmetric; }
    virtual void Eval(DenseMatrix &K, ElementTransformation &T, const IntegrationPoint &ip) = 0;
    virtual void SetTime(double t) { time = t; }
    double GetTime() const { return time; }

protected:
    int height, width;
    bool symmetric;
    double time = 0.0;
};

class MatrixConstantCoefficient : public MatrixCoefficient {
public:
    explicit MatrixConstantCoefficient(const DenseMatrix &m) : MatrixCoefficient(m.Height()), mat(m) {}
    void Eval(DenseMatrix &K, ElementTransformation &, const IntegrationPoint &) override { K = mat; }

private:
    DenseMatrix mat;
};

class MatrixFunctionCoefficient : public MatrixCoefficient {
public:
    MatrixFunctionCoefficient(int dim, std::function<void(const Vector &, DenseMatrix &)> f)
        : MatrixCoefficient(dim), f_(std::move(f)) {}
    void Eval(DenseMatrix &K, ElementTransformation &T, const IntegrationPoint &ip) override
    {
        Vector x;
        T.Transform(ip, x);
        K.SetSize(height);
        f_(x, K);
    }

private:
    std::function<void(const Vector &, DenseMatrix &)> f_;
};

// ---- command line (:245-253) -------------------------------------------------------------------
class OptionsParser {
public:
    OptionsParser(int argc, char *argv[]) : argc_(argc), argv_(argv) {}
    void AddOption(std::string *v, const char *s, const char *l, const char *d, bool req = false) { add(v, 's', s, l, d, req); }
    void AddOption(const char **v, const char *s, const char *l, const char *d, bool req = false) { add(v, 'c', s, l, d, req); }
    void AddOption(int *v, const char *s, const char *l, const char *d, bool req = false) { add(v, 'i', s, l, d, req); }
    void AddOption(double *v, const char *s, const char *l, const char *d, bool req = false) { add(v, 'd', s, l, d, req); }
    void AddOption(bool *v, const char *s, const char *l, const char *sn, const char *ln, const char *d,
                   bool req = false)
    {
        add(v, 'b', s, l, d, req);
        opts_.back().sn = sn;
        opts_.back().ln = ln;
    }
    void Parse()
    {
        good_ = true;
        for (int i = 1; i < argc_; ++i) {
            const std::string a = argv_[i];
            bool hit = false;
            for (Opt &o : opts_) {
                if (o.type == 'b' && (a == o.sn || a == o.ln)) {
                    *static_cast<bool *>(o.var) = false;
                    hit = o.seen = true;
                    break;
                }
                if (a != o.s && a != o.l) continue;
                hit = o.seen = true;
                if (o.type == 'b') {
                    *static_cast<bool *>(o.var) = true;
                    break;
                }
                if (i + 1 >= argc_) {
                    good_ = false;
                    return;
                }
                const char *v = argv_[++i];
                try {
                    switch (o.type) {
                    case 's': *static_cast<std::string *>(o.var) = v; break;
                    case 'c': *static_cast<const char **>(o.var) = v; break;
                    case 'i': *static_cast<int *>(o.var) = std::stoi(v); break;
                    case 'd': *static_cast<double *>(o.var) = std::stod(v); break;
                    }
                } catch (const std::exception &) {
                    good_ = false;
                    return;
                }
                break;
            }
            if (!hit) {
                good_ = false;
                return;
            }
        }
        for (const Opt &o : opts_)
            if (o.req && !o.seen) good_ = false;
    }
    bool Good() const { return good_; }
    void PrintUsage(std::ostream &os) const
    {
        os << "Usage: " << (argc_ > 0 ? argv_[0] : "driver") << " [options]\n";
        for (const Opt &o : opts_) os << "   " << o.s << ", " << o.l << "\n\t" << o.d << "\n";
    }
    void PrintOptions(std::ostream &os) const
    {
        os << "Options used:\n";
        for (const Opt &o : opts_) {
            os << "   " << o.l << " ";
            switch (o.type) {
            case 's': os << *static_cast<std::string *>(o.var); break;
            case 'c': os << (*static_cast<const char **>(o.var) ? *static_cast<const char **>(o.var) : ""); break;
            case 'i': os << *static_cast<int *>(o.var); break;
            case 'd': os << *static_cast<double *>(o.var); break;
            case 'b': os << (*static_cast<bool *>(o.var) ? "true" : "false"); break;
            }
            os << "\n";
        }
    }
    void PrintError(std::ostream &os) const { os << "invalid command line\n"; }

private:
    struct Opt {
        void *var;
        char type;
        std::string s, l, d, sn, ln;
        bool req, seen = false;
    };
    void add(void *v, char t, const char *s, const char *l, const char *d, bool req)
    {
        opts_.push_back(Opt{v, t, s ? s : "", l ? l : "", d ? d : "", "", "", req});
    }
    int argc_;
    char **argv_;
    std::vector<Opt> opts_;
    bool good_ = false;
};

// ---- mesh ------------------------------------------------------------------------------------------
struct Element {
    enum Type { POINT, SEGMENT, TRIANGLE, QUADRILATERAL, TETRAHEDRON, HEXAHEDRON, WEDGE, PYRAMID };
};

// A serial mesh: a structured box [0,sx] x [0,sy] (x [0,sz]) of quads / hexes (MFEM's Cartesian
// boundary attributes: 2D 1 bottom, 2 right, 3 top, 4 left; 3D 1 z=0, 2 y=0, 3 x=sx, 4 y=sy, 5 x=0,
// 6 z=sz), or a simplex mesh read from a gmsh v2.2 file (Mesh(mesh_file, 1, 1), :290).
class Mesh {
public:
    explicit Mesh(const char *path, int generate_edges = 1, int refine = 1, bool fix_orientation = true)
    {
        (void)generate_edges;
        (void)refine;
        (void)fix_orientation;
        cartesian_ = false;
        int ne = 0, nbe = 0;
        int64_t nv = 0;
        check(cdfem_gmsh_topology_sizes(path, &dim_, &nv, &ne, &nbe), nullptr,
              (std::string("cdfem_gmsh_topology_sizes (mesh file ") + path + ")").c_str());
        vxyz_.resize((size_t)nv * dim_);
        ev_.resize((size_t)ne * (dim_ + 1));
        bv_.resize((size_t)nbe * dim_);
        battr_.resize((size_t)nbe);
        check(cdfem_gmsh_topology(path, vxyz_.data(), ev_.data(), bv_.data(), battr_.data()), nullptr,
              "cdfem_gmsh_topology");
        SetAttributes();
    }
    explicit Mesh(const std::string &path, int generate_edges = 1, int refine = 1)
        : Mesh(path.c_str(), generate_edges, refine) {}
    static Mesh MakeCartesian2D(int nx, int ny, Element::Type, bool = false, double sx = 1.0, double sy = 1.0,
                                bool = true)
    {
        return Mesh(2, nx, ny, 1, sx, sy, 1.0);
    }
    static Mesh MakeCartesian3D(int nx, int ny, int nz, Element::Type, double sx = 1.0, double sy = 1.0,
                                double sz = 1.0, bool = true)
    {
        return Mesh(3, nx, ny, nz, sx, sy, sz);
    }
    Mesh(const Mesh &) = default;
    Mesh &operator=(const Mesh &) = default;
    virtual ~Mesh() = default;

    int Dimension() const { return dim_; }
    int SpaceDimension() const { return dim_; }
    virtual int GetNE() const { return GlobalNE(); }
    virtual int GetNV() const { return cartesian_ ? (int)LatticeVertices() : (int)(vxyz_.size() / dim_); }
    virtual const double *GetVertex(int i) const
    {
        if (!cartesian_) return &vxyz_[(size_t)i * dim_];
        const int64_t lx = n_[0] + 1, ly = n_[1] + 1;
        const int64_t ix = i % lx, iy = (i / lx) % ly, iz = i / (lx * ly);
        vbuf_[0] = s_[0] * (double)ix / n_[0];
        vbuf_[1] = s_[1] * (double)iy / n_[1];
        vbuf_[2] = dim_ == 3 ? s_[2] * (double)iz / n_[2] : 0.0;
        return vbuf_;
    }
    // boundary elements: the gmsh file's (segments in 2D, triangles in 3D), or the Cartesian box's
    // faces in MFEM's attribute order (2D: bottom, right, top, left; 3D: z=0, y=0, x=sx, y=sy, x=0,
    // z=sz)
    int GetNBE() const
    {
        if (!cartesian_) return (int)battr_.size();
        if (dim_ == 2) return 2 * (n_[0] + n_[1]);
        return 2 * (n_[0] * n_[1] + n_[0] * n_[2] + n_[1] * n_[2]);
    }
    int GetBdrAttribute(int i) const
    {
        if (i < 0 || i >= GetNBE()) throw std::out_of_range("GetBdrAttribute");
        if (!cartesian_) return battr_[(size_t)i];
        int a = 0, j = 0;
        CartesianFace(i, a, j);
        return a;
    }
    ElementTransformation *GetBdrElementTransformation(int i) const
    {
        if (i < 0 || i >= GetNBE()) throw std::out_of_range("GetBdrElementTransformation");
        double X0[3] = {0, 0, 0}, E0[3] = {0, 0, 0}, E1[3] = {0, 0, 0};
        if (!cartesian_) {
            const int nv = dim_;  // vertices per boundary element
            const int32_t *b = &bv_[(size_t)i * nv];
            for (int k = 0; k < dim_; ++k) {
                X0[k] = vxyz_[(size_t)b[0] * dim_ + k];
                E0[k] = vxyz_[(size_t)b[1] * dim_ + k] - X0[k];
                if (nv == 3) E1[k] = vxyz_[(size_t)b[2] * dim_ + k] - X0[k];
            }
            btr_.SetAffine(dim_, dim_ == 2 ? Geometry::SEGMENT : Geometry::TRIANGLE, X0, E0, nv == 3 ? E1 : nullptr);
        } else {
            int a = 0, j = 0;
            CartesianFace(i, a, j);
            // the face's fixed axis / position and its two running axes
            static const int fixed3[6] = {2, 1, 0, 1, 0, 2}, fixed2[4] = {1, 0, 1, 0};
            const int fx = dim_ == 2 ? fixed2[a - 1] : fixed3[a - 1];
            const bool hi = dim_ == 2 ? (a == 2 || a == 3) : (a == 3 || a == 4 || a == 6);
            int run[2] = {-1, -1}, nr = 0;
            for (int k = 0; k < dim_; ++k)
                if (k != fx) run[nr++] = k;
            X0[fx] = hi ? s_[fx] : 0.0;
            const int i0 = j % n_[run[0]], i1 = nr > 1 ? j / n_[run[0]] : 0;
            const double h0 = s_[run[0]] / n_[run[0]];
            X0[run[0]] = i0 * h0;
            E0[run[0]] = h0;
            if (nr > 1) {
                const double h1 = s_[run[1]] / n_[run[1]];
                X0[run[1]] = i1 * h1;
                E1[run[1]] = h1;
            }
            btr_.SetAffine(dim_, dim_ == 2 ? Geometry::SEGMENT : Geometry::SQUARE, X0, E0, nr > 1 ? E1 : nullptr);
        }
        btr_.ElementNo = i;
        btr_.Attribute = GetBdrAttribute(i);
        return &btr_;
    }
    // uniform refinement: boxes halve h; triangles split into 4 (red refinement), boundary segments in 2
    virtual void UniformRefinement() { Refine(nullptr); }

    // -- library-side description --
    bool Cartesian() const { return cartesian_; }
    int N(int k) const { return n_[k]; }
    double Size(int k) const { return s_[k]; }
    int GlobalNE() const
    {
        return cartesian_ ? (dim_ == 3 ? n_[0] * n_[1] * n_[2] : n_[0] * n_[1]) : (int)(ev_.size() / (dim_ + 1));
    }
    const std::vector<double> &TopoVertices() const { return vxyz_; }
    const std::vector<int32_t> &TopoElements() const { return ev_; }
    const std::vector<int32_t> &TopoBoundary() const { return bv_; }
    const std::vector<int32_t> &TopoBoundaryAttr() const { return battr_; }
    // element centroids (the partitioner's input)
    std::vector<double> Centroids() const
    {
        const int ne = GlobalNE();
        std::vector<double> c((size_t)ne * dim_, 0.0);
        for (int e = 0; e < ne; ++e) {
            if (cartesian_) {
                const int ix = e % n_[0], iy = (e / n_[0]) % n_[1], iz = e / (n_[0] * n_[1]);
                const int ii[3] = {ix, iy, iz};
                for (int k = 0; k < dim_; ++k) c[(size_t)e * dim_ + k] = s_[k] * (ii[k] + 0.5) / n_[k];
            } else {
                for (int v = 0; v <= dim_; ++v)
                    for (int k = 0; k < dim_; ++k)
                        c[(size_t)e * dim_ + k] += vxyz_[(size_t)ev_[(size_t)e * (dim_ + 1) + v] * dim_ + k] / (dim_ + 1);
            }
        }
        return c;
    }

    Array<int> bdr_attributes;

protected:
    Mesh() = default;
    Mesh(int dim, int nx, int ny, int nz, double sx, double sy, double sz) : dim_(dim), n_{nx, ny, nz}, s_{sx, sy, sz}
    {
        if (nx < 1 || ny < 1 || nz < 1) throw std::invalid_argument("Mesh: element counts must be >= 1");
        SetAttributes();
    }
    // Cartesian boundary element i -> attribute a and its index j within that face
    void CartesianFace(int i, int &a, int &j) const
    {
        int cnt[6];
        if (dim_ == 2) {
            cnt[0] = n_[0]; cnt[1] = n_[1]; cnt[2] = n_[0]; cnt[3] = n_[1];
        } else {
            cnt[0] = n_[0] * n_[1]; cnt[1] = n_[0] * n_[2]; cnt[2] = n_[1] * n_[2];
            cnt[3] = n_[0] * n_[2]; cnt[4] = n_[1] * n_[2]; cnt[5] = n_[0] * n_[1];
        }
        j = i;
        for (a = 1; a <= 2 * dim_; ++a) {
            if (j < cnt[a - 1]) return;
            j -= cnt[a - 1];
        }
        throw std::out_of_range("boundary element");
    }
    int64_t LatticeVertices() const
    {
        return (int64_t)(n_[0] + 1) * (n_[1] + 1) * (dim_ == 3 ? n_[2] + 1 : 1);
    }
    void SetAttributes()
    {
        bdr_attributes.SetSize(0);
        if (cartesian_) {
            for (int a = 1; a <= 2 * dim_; ++a) bdr_attributes.Append(a);
            return;
        }
        std::vector<int32_t> a(battr_);
        std::sort(a.begin(), a.end());
        a.erase(std::unique(a.begin(), a.end()), a.end());
        for (int32_t v : a) bdr_attributes.Append(v);
    }
    // refine; parent_of (if given) receives, per new element, its parent element
    void Refine(std::vector<int32_t> *parent_of)
    {
        const int ne = GlobalNE();
        if (cartesian_) {
            const int o[3] = {n_[0], n_[1], n_[2]};
            for (int k = 0; k < dim_; ++k) n_[k] *= 2;
            if (parent_of) {
                parent_of->resize((size_t)GlobalNE());
                for (int e = 0; e < GlobalNE(); ++e) {
                    const int ix = e % n_[0], iy = (e / n_[0]) % n_[1], iz = e / (n_[0] * n_[1]);
                    (*parent_of)[e] = ix / 2 + o[0] * (iy / 2 + o[1] * (dim_ == 3 ? iz / 2 : 0));
                }
            }
            return;
        }
        if (dim_ != 2) throw std::invalid_argument("UniformRefinement: tetrahedral refinement is not provided");
        std::map<std::pair<int32_t, int32_t>, int32_t> mid;
        auto midpoint = [&](int32_t a, int32_t b) {
            const auto key = std::make_pair(std::min(a, b), std::max(a, b));
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const int32_t id = (int32_t)(vxyz_.size() / 2);
            vxyz_.push_back(0.5 * (vxyz_[(size_t)a * 2] + vxyz_[(size_t)b * 2]));
            vxyz_.push_back(0.5 * (vxyz_[(size_t)a * 2 + 1] + vxyz_[(size_t)b * 2 + 1]));
            mid.emplace(key, id);
            return id;
        };
        std::vector<int32_t> ev;
        ev.reserve((size_t)ne * 12);
        if (parent_of) parent_of->clear();
        for (int e = 0; e < ne; ++e) {
            const int32_t v0 = ev_[(size_t)e * 3], v1 = ev_[(size_t)e * 3 + 1], v2 = ev_[(size_t)e * 3 + 2];
            const int32_t m01 = midpoint(v0, v1), m12 = midpoint(v1, v2), m02 = midpoint(v0, v2);
            const int32_t kids[4][3] = {{v0, m01, m02}, {m01, v1, m12}, {m02, m12, v2}, {m01, m12, m02}};
            for (auto &k : kids) {
                ev.insert(ev.end(), k, k + 3);
                if (parent_of) parent_of->push_back(e);
            }
        }
        std::vector<int32_t> bv, ba;
        for (size_t b = 0; b < battr_.size(); ++b) {
            const int32_t a = bv_[b * 2], c = bv_[b * 2 + 1], m = midpoint(a, c);
            bv.insert(bv.end(), {a, m, m, c});
            ba.insert(ba.end(), {battr_[b], battr_[b]});
        }
        ev_.swap(ev);
        bv_.swap(bv);
        battr_.swap(ba);
    }

    int dim_ = 0;
    bool cartesian_ = true;
    int n_[3] = {1, 1, 1};
    double s_[3] = {1.0, 1.0, 1.0};
    std::vector<double> vxyz_;
    std::vector<int32_t> ev_, bv_, battr_;
    mutable double vbuf_[3] = {0, 0, 0};
    mutable ElementTransformation btr_;
};

// ParMesh(MPI_COMM_WORLD, *mesh) (:300): the ranks' share of the elements.  A 3D box whose z element
// count divides by the rank count is split into z-slabs (the structured kernels run on each slab);
// any other mesh is split by recursive coordinate bisection of the element centroids
// (cdfem_partition_rcb; MFEM uses METIS — any partition gives the same global operator).
// UniformRefinement after the split keeps every child on its parent's rank, as MFEM's ParMesh does.
class ParMesh : public Mesh {
public:
    ParMesh(MPI_Comm comm, Mesh &mesh, const int *partitioning = nullptr, int part_method = 1)
        : Mesh(mesh), comm_(comm)
    {
        (void)part_method;
        rank_ = detail::comm_rank(comm);
        size_ = detail::comm_size(comm);
        const int ne = GlobalNE();
        if (size_ > ne) throw std::invalid_argument("ParMesh: more ranks than elements");
        slab_ = size_ > 1 && !partitioning && Cartesian() && dim_ == 3 && n_[2] % size_ == 0;
        if (size_ > 1 && !slab_) {
            part_.resize((size_t)ne);
            if (partitioning) {
                std::copy(partitioning, partitioning + ne, part_.begin());
            } else {
                // the partitioner takes element vertex arrays; centroids as one-vertex "elements"
                const std::vector<double> c = Centroids();
                check(cdfem_partition_rcb(dim_, ne, 1, c.data(), size_, part_.data()), nullptr, "cdfem_partition_rcb");
            }
        }
    }
    MPI_Comm GetComm() const { return comm_; }
    int GetMyRank() const { return rank_; }
    int GetNRanks() const { return size_; }
    bool Slab() const { return slab_; }
    const std::vector<int32_t> &Partition() const { return part_; }
    // slab: elements [z0, z1) along z
    int SlabZ0() const { return rank_ * (n_[2] / size_); }
    int SlabZ1() const { return (rank_ + 1) * (n_[2] / size_); }

    int GetNE() const override
    {
        if (size_ == 1) return GlobalNE();
        if (slab_) return n_[0] * n_[1] * (n_[2] / size_);
        return (int)std::count(part_.begin(), part_.end(), rank_);
    }
    // the vertices of this rank's elements (MFEM's ParMesh vertex set), first-use order
    int GetNV() const override
    {
        LocalVertices();
        return (int)lverts_.size() / dim_;
    }
    const double *GetVertex(int i) const override
    {
        LocalVertices();
        return &lverts_[(size_t)i * dim_];
    }
    void UniformRefinement() override
    {
        std::vector<int32_t> parent;
        Refine(size_ > 1 && !slab_ ? &parent : nullptr);
        if (!parent.empty()) {
            std::vector<int32_t> p(parent.size());
            for (size_t e = 0; e < parent.size(); ++e) p[e] = part_[(size_t)parent[e]];
            part_.swap(p);
        }
        lverts_.clear();
    }

private:
    void LocalVertices() const
    {
        if (!lverts_.empty()) return;
        if (size_ == 1) {
            for (int i = 0; i < Mesh::GetNV(); ++i) lverts_.insert(lverts_.end(), Mesh::GetVertex(i), Mesh::GetVertex(i) + dim_);
            return;
        }
        if (Cartesian()) {
            const int64_t lx = n_[0] + 1, ly = n_[1] + 1, lz = dim_ == 3 ? n_[2] + 1 : 1;
            std::vector<char> used((size_t)(lx * ly * lz), 0);
            for (int e = 0; e < GlobalNE(); ++e) {
                const int ix = e % n_[0], iy = (e / n_[0]) % n_[1], iz = e / (n_[0] * n_[1]);
                const bool mine = slab_ ? (iz >= SlabZ0() && iz < SlabZ1()) : part_[(size_t)e] == rank_;
                if (!mine) continue;
                for (int c = 0; c < (1 << dim_); ++c)
                    used[(size_t)((ix + (c & 1)) + lx * ((iy + ((c >> 1) & 1)) + ly * (dim_ == 3 ? iz + ((c >> 2) & 1) : 0)))] = 1;
            }
            for (int64_t v = 0; v < (int64_t)used.size(); ++v)
                if (used[(size_t)v]) lverts_.insert(lverts_.end(), Mesh::GetVertex((int)v), Mesh::GetVertex((int)v) + dim_);
            return;
        }
        std::vector<char> used(vxyz_.size() / dim_, 0);
        for (int e = 0; e < GlobalNE(); ++e)
            if (part_[(size_t)e] == rank_)
                for (int v = 0; v <= dim_; ++v) used[(size_t)ev_[(size_t)e * (dim_ + 1) + v]] = 1;
        for (size_t v = 0; v < used.size(); ++v)
            if (used[v]) lverts_.insert(lverts_.end(), &vxyz_[v * dim_], &vxyz_[v * dim_] + dim_);
    }
    MPI_Comm comm_;
    int rank_ = 0, size_ = 1;
    bool slab_ = false;
    std::vector<int32_t> part_;
    mutable std::vector<double> lverts_;
};

class H1_FECollection {
public:
    H1_FECollection(int p, int dim, int btype = 1) : p_(p), dim_(dim)
    {
        (void)btype;  // GaussLobatto nodal basis (MFEM's default BasisType)
        if (p < 1) throw std::invalid_argument("H1_FECollection: order must be >= 1");
    }
    int GetOrder() const { return p_; }
    int GetDim() const { return dim_; }

private:
    int p_, dim_;
};

class DeviceSpace;

// The rank-local H1 space: local element arrays, local L-dofs (dofs owned by a lower rank first),
// the partition the library needs (z-slab flags or shared-dof lists), and one device context with
// the mesh and the communicator for linear forms, prolongation and the essential-dof map.
class FiniteElementSpace {
public:
    FiniteElementSpace(Mesh *mesh, H1_FECollection *fec, int vdim = 1, int ordering = 0) : mesh_(mesh), fec_(fec), vdim_(vdim)
    {
        (void)ordering;
        if (mesh->Dimension() != fec->GetDim()) throw std::invalid_argument("FiniteElementSpace: dim mismatch");
        pmesh_ = dynamic_cast<ParMesh *>(mesh);
        nranks_ = pmesh_ ? pmesh_->GetNRanks() : 1;
        rank_ = pmesh_ ? pmesh_->GetMyRank() : 0;
        const int dim = mesh->Dimension(), p = fec->GetOrder();
        if (mesh->Cartesian()) {
            const int z0 = (pmesh_ && pmesh_->Slab()) ? pmesh_->SlabZ0() : 0;
            const int z1 = (pmesh_ && pmesh_->Slab()) ? pmesh_->SlabZ1() : 0;
            int ne = 0, ness = 0;
            int64_t nl = 0;
            check(cdfem_box_sizes(dim, mesh->N(0), mesh->N(1), mesh->N(2), p, z0, z1, &ne, &nl, &ness), nullptr,
                  "cdfem_box_sizes");
            ne_ = ne;
            nl_ = (int)nl;
            nv_ = 1 << dim;
            nd_ = dim == 3 ? (p + 1) * (p + 1) * (p + 1) : (p + 1) * (p + 1);
            verts_.resize((size_t)ne_ * nv_ * dim);
            dofs_.resize((size_t)ne_ * nd_);
            std::vector<int32_t> ess((size_t)ness);
            xyz_.resize((size_t)nl_ * dim);
            check(cdfem_box_mesh(dim, mesh->N(0), mesh->N(1), mesh->N(2), p, z0, z1, 0.0, verts_.data(), dofs_.data(),
                                 ess.data(), xyz_.data()),
                  nullptr, "cdfem_box_mesh");
            for (size_t i = 0; i < verts_.size(); ++i) verts_[i] *= mesh->Size((int)(i % dim));
            for (size_t i = 0; i < xyz_.size(); ++i) xyz_[i] *= mesh->Size((int)(i % dim));
            structured_ = dim == 3 && (nranks_ == 1 || pmesh_->Slab());
            sz_ = z1 > z0 ? z1 - z0 : mesh->N(2);
            if (pmesh_ && pmesh_->Slab()) {
                slab_lo_ = rank_ > 0;
                slab_hi_ = rank_ < nranks_ - 1;
                n_not_owned_ = slab_lo_ ? (int64_t)(p * mesh->N(0) + 1) * (p * mesh->N(1) + 1) : 0;
                return;
            }
        } else {
            simplex_ = true;
            const std::vector<double> &V = mesh->TopoVertices();
            const std::vector<int32_t> &E = mesh->TopoElements(), &BV = mesh->TopoBoundary(), &BA = mesh->TopoBoundaryAttr();
            const int64_t nvert = (int64_t)V.size() / dim;
            const int ne = (int)(E.size() / (dim + 1));
            int64_t nl = 0;
            check(cdfem_simplex_space_sizes(dim, nvert, V.data(), ne, E.data(), p, &nl), nullptr,
                  "cdfem_simplex_space_sizes (order / mesh)");
            ne_ = ne;
            nl_ = (int)nl;
            nv_ = dim + 1;
            nd_ = p == 1 ? dim + 1 : p == 2 ? (dim + 1) * (dim + 2) / 2 : 10;
            verts_.resize((size_t)ne_ * nv_ * dim);
            dofs_.resize((size_t)ne_ * nd_);
            xyz_.resize((size_t)nl_ * dim);
            bmask_.resize((size_t)nl_);
            check(cdfem_simplex_space(dim, nvert, V.data(), ne, E.data(), (int)BA.size(), BV.data(), BA.data(), p,
                                      verts_.data(), dofs_.data(), bmask_.data(), xyz_.data()),
                  nullptr, "cdfem_simplex_space");
        }
        if (nranks_ > 1) Localize();
    }
    Mesh *GetMesh() const { return mesh_; }
    ParMesh *GetParMesh() const { return pmesh_; }
    int GetOrder() const { return fec_->GetOrder(); }
    int GetVDim() const { return vdim_; }
    int GetVSize() const { return vdim_ * nl_; }
    int GetTrueVSize() const { return vdim_ * (nl_ - (int)n_not_owned_); }
    int TrueVSize() const { return GetTrueVSize(); }
    HYPRE_BigInt GlobalTrueVSize() const
    {
        return (HYPRE_BigInt)std::llround(detail::allreduce_sum((double)GetTrueVSize(), Comm()));
    }
    int GetNE() const { return ne_; }
    MPI_Comm Comm() const { return pmesh_ ? pmesh_->GetComm() : MPI_COMM_WORLD; }
    int NRanks() const { return nranks_; }
    int64_t FirstOwned() const { return n_not_owned_; }

    // true dofs on the boundary faces whose attribute is marked (ess_bdr[attr - 1] != 0), as
    // MFEM's ParFiniteElementSpace::GetEssentialTrueDofs: indices into the true-dof vector
    void GetEssentialTrueDofs(const Array<int> &ess_bdr, Array<int> &list) const
    {
        const int dim = mesh_->Dimension();
        list.SetSize(0);
        for (int i = (int)n_not_owned_; i < nl_; ++i)
            if (OnMarkedBoundary(i, ess_bdr, dim)) list.Append(i - (int)n_not_owned_);
    }
    // L-dof marker of a boundary selection (local numbering, shared dofs included)
    void GetEssentialVDofs(const Array<int> &ess_bdr, Array<int> &marker) const
    {
        marker.SetSize(nl_);
        for (int i = 0; i < nl_; ++i) marker[i] = OnMarkedBoundary(i, ess_bdr, mesh_->Dimension()) ? -1 : 0;
    }
    bool OnMarkedBoundary(int i, const Array<int> &marker, int dim) const
    {
        if (simplex_) {
            // attributes above 31 cannot occur: the gmsh reader and cdfem_simplex_space reject them
            for (int a = 1; a <= marker.Size() && a <= 31; ++a)
                if (marker[a - 1] && (bmask_[(size_t)i] & (1 << (a - 1)))) return true;
            return false;
        }
        const double *X = &xyz_[(size_t)i * dim];
        auto at = [&](int attr) { return attr <= marker.Size() && marker[attr - 1] != 0; };
        const double sx = mesh_->Size(0), sy = mesh_->Size(1), sz = mesh_->Size(2);
        if (dim == 2)
            return (X[1] == 0.0 && at(1)) || (X[0] == sx && at(2)) || (X[1] == sy && at(3)) || (X[0] == 0.0 && at(4));
        return (X[2] == 0.0 && at(1)) || (X[1] == 0.0 && at(2)) || (X[0] == sx && at(3)) || (X[1] == sy && at(4)) ||
               (X[0] == 0.0 && at(5)) || (X[2] == sz && at(6));
    }
    const std::vector<double> &ElementVertices() const { return verts_; }
    const std::vector<int32_t> &ElementDofs() const { return dofs_; }
    const std::vector<double> &DofCoordinates() const { return xyz_; }
    bool Simplex() const { return simplex_; }
    bool Structured() const { return structured_; }
    int StructuredNz() const { return sz_; }
    int NumElementDofs() const { return nd_; }
    bool SlabLo() const { return slab_lo_; }
    bool SlabHi() const { return slab_hi_; }
    bool SlabPartition() const { return pmesh_ && pmesh_->Slab(); }
    const std::vector<int32_t> &NbrRanks() const { return nbr_ranks_; }
    const std::vector<int64_t> &NbrOff() const { return nbr_off_; }
    const std::vector<int32_t> &NbrIdx() const { return nbr_idx_; }
    const std::vector<int64_t> &L2G() const { return l2g_; }  // global id of each local dof
    // the space's device context (mesh + communicator, no operator), created on first use
    DeviceSpace &Space() const;

private:
    // general partition: keep this rank's elements and dofs (cdfem_local_space)
    void Localize()
    {
        const int dim = mesh_->Dimension();
        const std::vector<int32_t> &part = pmesh_->Partition();
        int neloc = 0, nnbr = 0;
        int64_t nlloc = 0, nsh = 0, nno = 0;
        check(cdfem_local_space_sizes(ne_, nd_, nl_, dofs_.data(), part.data(), rank_, &neloc, &nlloc, &nnbr, &nsh, &nno),
              nullptr, "cdfem_local_space_sizes");
        std::vector<int32_t> elems((size_t)neloc), ldofs((size_t)neloc * nd_);
        std::vector<int64_t> l2g((size_t)nlloc);
        nbr_ranks_.resize((size_t)nnbr);
        nbr_off_.resize((size_t)nnbr + 1);
        nbr_idx_.resize((size_t)std::max<int64_t>(nsh, 1));
        check(cdfem_local_space(ne_, nd_, nl_, dofs_.data(), part.data(), rank_, elems.data(), ldofs.data(), l2g.data(),
                                nbr_ranks_.data(), nbr_off_.data(), nbr_idx_.data()),
              nullptr, "cdfem_local_space");
        nbr_idx_.resize((size_t)nsh);
        std::vector<double> v((size_t)neloc * nv_ * dim), x((size_t)nlloc * dim);
        std::vector<int32_t> bm(simplex_ ? (size_t)nlloc : 0);
        for (int e = 0; e < neloc; ++e)
            std::copy(&verts_[(size_t)elems[e] * nv_ * dim], &verts_[(size_t)(elems[e] + 1) * nv_ * dim], &v[(size_t)e * nv_ * dim]);
        for (int64_t i = 0; i < nlloc; ++i) {
            std::copy(&xyz_[(size_t)l2g[i] * dim], &xyz_[(size_t)(l2g[i] + 1) * dim], &x[(size_t)i * dim]);
            if (simplex_) bm[(size_t)i] = bmask_[(size_t)l2g[i]];
        }
        verts_.swap(v);
        xyz_.swap(x);
        bmask_.swap(bm);
        dofs_.swap(ldofs);
        ne_ = neloc;
        nl_ = (int)nlloc;
        n_not_owned_ = nno;
        l2g_.swap(l2g);
        structured_ = false;
    }

    mutable std::shared_ptr<DeviceSpace> space_;
    Mesh *mesh_;
    ParMesh *pmesh_ = nullptr;
    H1_FECollection *fec_;
    int vdim_ = 1, nranks_ = 1, rank_ = 0;
    int ne_ = 0, nl_ = 0, nv_ = 0, nd_ = 0, sz_ = 1;
    int64_t n_not_owned_ = 0;
    std::vector<int64_t> l2g_;  // general partition: global id of each local dof
    bool simplex_ = false, structured_ = false, slab_lo_ = false, slab_hi_ = false;
    std::vector<double> verts_, xyz_;
    std::vector<int32_t> dofs_, bmask_;
    std::vector<int32_t> nbr_ranks_, nbr_idx_;
    std::vector<int64_t> nbr_off_;
};
using ParFiniteElementSpace = FiniteElementSpace;

// ---- device context (one cdfem_ctx: mesh, partition and communicator resident on the GPU) -----------
class DeviceSpace {
public:
    explicit DeviceSpace(const FiniteElementSpace &fes)
    {
        if (fes.GetVDim() != 1) throw std::invalid_argument("forms on vector spaces (vdim > 1) are not provided");
        check(cdfem_create(detail::device_id(), &ctx_), nullptr, "cdfem_create (no GPU? there is no CPU path)");
        if (fes.NRanks() > 1) check(cdfem_comm_share(ctx_, detail::comm_anchor()), ctx_, "cdfem_comm_share");
        Upload(fes, std::vector<int32_t>());
    }
    ~DeviceSpace() { cdfem_destroy(ctx_); }
    DeviceSpace(const DeviceSpace &) = delete;
    DeviceSpace &operator=(const DeviceSpace &) = delete;
    // the space with an essential L-dof list (the constraint is part of the resident operator)
    void Upload(const FiniteElementSpace &fes, const std::vector<int32_t> &ess)
    {
        Mesh *m = fes.GetMesh();
        const int dim = m->Dimension();
        simplex_ = fes.Simplex();
        points_.clear();
        auto up = simplex_ ? cdfem_mesh_upload_simplex : cdfem_mesh_upload;
        check(up(ctx_, dim, fes.GetOrder(), fes.GetNE(), fes.ElementVertices().data(), fes.GetVSize(),
                 fes.ElementDofs().data(), (int)ess.size(), ess.data()),
              ctx_, simplex_ ? "cdfem_mesh_upload_simplex" : "cdfem_mesh_upload");
        // the Cartesian box is lexicographic: the structured fast paths (bricks p <= 2, lattice E->L p >= 3)
        if (fes.Structured())
            check(cdfem_mesh_set_structured(ctx_, m->N(0), m->N(1), fes.StructuredNz()), ctx_, "cdfem_mesh_set_structured");
        if (fes.NRanks() > 1) {
            if (fes.SlabPartition()) {
                check(cdfem_set_slab(ctx_, fes.SlabLo(), fes.SlabHi()), ctx_, "cdfem_set_slab");
            } else {
                const auto &r = fes.NbrRanks();
                const auto &o = fes.NbrOff();
                const auto &ix = fes.NbrIdx();
                check(cdfem_set_shared(ctx_, (int)r.size(), r.data(), o.data(), ix.empty() ? nullptr : ix.data()), ctx_,
                      "cdfem_set_shared");
                check(cdfem_check_shared(ctx_, fes.L2G().data()), ctx_, "cdfem_check_shared");
            }
        }
        ess_ = ess;
    }
    cdfem_ctx *ctx() const { return ctx_; }
    const std::vector<int32_t> &Ess() const { return ess_; }
    bool Simplex() const { return simplex_; }
    // physical coordinates of a rule's points, element-major; kept per rule (a time loop's linear
    // form samples its coefficient at the same points every step)
    const std::vector<double> &Points(int rule, int dim, int ne, int &nq) const
    {
        auto it = points_.find(rule);
        if (it == points_.end()) {
            int n = 0;
            check(cdfem_rule_size(ctx_, rule, &n), ctx_, "cdfem_rule_size");
            std::vector<double> xyz((size_t)ne * n * dim);
            check(cdfem_quadrature_points(ctx_, rule, xyz.data(), CDFEM_HOST), ctx_, "cdfem_quadrature_points");
            it = points_.emplace(rule, std::make_pair(n, std::move(xyz))).first;
        }
        nq = it->second.first;
        return it->second.second;
    }
    // x (L) = P X (true dofs), host arrays
    void Prolongate(const double *X, double *x) const
    {
        check(cdfem_prolongate(ctx_, X, x, CDFEM_HOST), ctx_, "cdfem_prolongate");
    }
    // the same on device vectors
    void Prolongate(const Vector &X, Vector &x) const
    {
        check(cdfem_prolongate(ctx_, X.Read(), x.Write(), CDFEM_DEVICE), ctx_, "cdfem_prolongate");
    }

private:
    cdfem_ctx *ctx_ = nullptr;
    std::vector<int32_t> ess_;
    bool simplex_ = false;
    mutable std::map<int, std::pair<int, std::vector<double>>> points_;
};

inline DeviceSpace &FiniteElementSpace::Space() const
{
    if (!space_) space_ = std::make_shared<DeviceSpace>(*this);
    return *space_;
}

// sample a scalar coefficient at the given points (host virtual calls, as in MFEM)
inline std::vector<double> Sample(Coefficient &q, const std::vector<double> &xyz, int dim, int nq)
{
    ElementTransformation T;
    IntegrationPoint ip;
    const size_t n = xyz.size() / dim;
    std::vector<double> out(n);
    for (size_t i = 0; i < n; ++i) {
        T.ElementNo = (int)(i / nq);
        T.SetPoint(dim, &xyz[i * dim]);
        out[i] = q.Eval(T, ip);
    }
    return out;
}

// ---- operators -----------------------------------------------------------------------------------
class Operator {
public:
    enum Type { ANY_TYPE, MFEM_SPARSEMAT, Hypre_ParCSR, PETSC_MATAIJ, PETSC_MATIS, PETSC_MATSHELL, PETSC_MATNEST,
                PETSC_MATHYPRE, PETSC_MATGENERIC };
    Operator(int h = 0, int w = 0) : height(h), width(w) {}
    virtual ~Operator() = default;
    virtual void Mult(const Vector &x, Vector &y) const = 0;
    int Height() const { return height; }
    int Width() const { return width; }

protected:
    int height, width;
};

class BilinearForm;

// the operator FormLinearSystem returns: P^T A P on the true dofs with the essential rows and
// columns eliminated (DIAG_ONE), held on the GPU (PA ConstrainedOperator / FA eliminated CSR)
class ConstrainedPAOperator : public Operator {
public:
    ConstrainedPAOperator(const BilinearForm *a, int n) : Operator(n, n), a_(a) {}
    void Mult(const Vector &x, Vector &y) const override;
    const BilinearForm *Form() const { return a_; }

private:
    const BilinearForm *a_;
};
// the reference casts the FormLinearSystem result to HypreParMatrix (:364): the same object here
using HypreParMatrix = ConstrainedPAOperator;

class OperatorHandle {
public:
    OperatorHandle() = default;
    explicit OperatorHandle(Operator::Type t) : type_(t) {}
    void Reset(Operator *op) { op_ = op; }
    Operator *Ptr() const { return op_; }
    Operator *operator->() const { return op_; }
    Operator &operator*() const { return *op_; }
    template <class T>
    T *As() const { return dynamic_cast<T *>(op_); }
    Operator::Type Type() const { return type_; }

private:
    Operator *op_ = nullptr;
    Operator::Type type_ = Operator::ANY_TYPE;
};

// ---- integrators --------------------------------------------------------------------------------
class BilinearFormIntegrator {
public:
    virtual ~BilinearFormIntegrator() = default;
    virtual unsigned Kind() const = 0;
};

class DiffusionIntegrator : public BilinearFormIntegrator {
public:
    DiffusionIntegrator() = default;
    explicit DiffusionIntegrator(Coefficient &q) : Q_(&q) {}
    explicit DiffusionIntegrator(MatrixCoefficient &m) : MQ_(&m) {}
    unsigned Kind() const override { return CDFEM_DIFFUSION; }
    Coefficient *Q_ = nullptr;
    MatrixCoefficient *MQ_ = nullptr;
};

class ConvectionIntegrator : public BilinearFormIntegrator {
public:
    explicit ConvectionIntegrator(VectorCoefficient &q, double a = 1.0) : Q_(&q), alpha(a) {}
    unsigned Kind() const override { return CDFEM_CONVECTION; }
    VectorCoefficient *Q_;
    double alpha;
};

class MassIntegrator : public BilinearFormIntegrator {
public:
    MassIntegrator() = default;
    explicit MassIntegrator(Coefficient &q) : Q_(&q) {}
    unsigned Kind() const override { return CDFEM_MASS; }
    Coefficient *Q_ = nullptr;
};

enum class AssemblyLevel { LEGACY, FULL, ELEMENT, PARTIAL, NONE };

class GridFunction;

class BilinearForm : public Operator {
public:
    explicit BilinearForm(FiniteElementSpace *f) : Operator(f->GetVSize(), f->GetVSize()), fes_(f) {}
    // the form takes ownership of the integrator (MFEM semantics, :336-338)
    void AddDomainIntegrator(BilinearFormIntegrator *bfi) { integs_.emplace_back(bfi); }
    // simplices: full assembly on the GPU whatever the level.  Hexes / quads: partial assembly unless LEGACY or
    // FULL is asked for explicitly, which assembles the CSR operator (cdfem_fa_setup_form: one rank, quads
    // p = 1..4, hexes p = 1, 2); no call, PARTIAL, ELEMENT and NONE keep partial assembly
    void SetAssemblyLevel(AssemblyLevel l) { level_ = l; level_set_ = true; }
    // the resident operator is (or will be, once assembled) a CSR matrix: what ILU(0) needs
    bool Assembled() const
    {
        return fes_->Simplex() || (level_set_ && (level_ == AssemblyLevel::LEGACY || level_ == AssemblyLevel::FULL));
    }
    FiniteElementSpace *FESpace() const { return fes_; }

    void Assemble(int = 1)
    {
        if (!dev_) dev_ = std::make_unique<DeviceSpace>(*fes_);
        Setup();
    }
    void Finalize(int = 1) {}

    // y = A x on rank-local L-vectors without the shared-dof exchange (BilinearForm::Mult on a
    // ParBilinearForm, diffusion_mms.cpp:430: a partial L-vector, summed later by FormLinearSystem)
    void Mult(const Vector &x, Vector &y) const override
    {
        Require(x.Size() == height, "Mult: size");
        y.SetSize(height);
        check(cdfem_pa_mult(ctx(), x.Read(), y.Write(), 2, CDFEM_DEVICE), ctx(), "cdfem_pa_mult");
        check(cdfem_synchronize(ctx()), ctx(), "cdfem_synchronize");
    }

    // FormLinearSystem (:349-351): X = R x, B = P^T (b - A x_e) with B_ess = x_ess, both true-dof
    // vectors; A = the constrained P^T A P
    void FormLinearSystem(const Array<int> &ess_tdof_list, Vector &x, Vector &b, OperatorHandle &A, Vector &X,
                          Vector &B)
    {
        Require(x.Size() == height && b.Size() == height, "FormLinearSystem: size");
        if (!dev_) throw std::logic_error("FormLinearSystem before Assemble");
        const std::vector<int32_t> ess = EssentialLDofs(ess_tdof_list);
        if (ess != dev_->Ess()) {  // the constraint is part of the resident operator
            dev_->Upload(*fes_, ess);
            Setup();
        }
        const int nt = fes_->GetTrueVSize(), off = (int)fes_->FirstOwned();
        if (fes_->NRanks() == 1) {  // one rank: the true dofs are the L-dofs (P = I)
            X.SetSize(nt);
            B.SetSize(nt);
            check(cdfem_form_linear_system(ctx(), x.Read(), b.Read(), X.Write(), B.Write(), CDFEM_DEVICE), ctx(),
                  "cdfem_form_linear_system");
        } else {
            XL_.SetSize(height);
            BL_.SetSize(height);
            check(cdfem_form_linear_system(ctx(), x.Read(), b.Read(), XL_.Write(), BL_.Write(), CDFEM_DEVICE), ctx(),
                  "cdfem_form_linear_system");
            X.SetSubVectorOf(XL_, off, nt);
            B.SetSubVectorOf(BL_, off, nt);
        }
        cop_ = std::make_unique<ConstrainedPAOperator>(this, nt);
        A.Reset(cop_.get());
    }

    // x = P X (:377)
    void RecoverFEMSolution(const Vector &X, const Vector &, Vector &x) const
    {
        Require(X.Size() == fes_->GetTrueVSize(), "RecoverFEMSolution: size");
        x.SetSize(height);
        dev_->Prolongate(X, x);
    }

    cdfem_ctx *ctx() const { return dev_->ctx(); }
    const DeviceSpace &DeviceCtx() const { return *dev_; }

private:
    static void Require(bool ok, const char *what)
    {
        if (!ok) throw std::invalid_argument(what);
    }
    // essential true dofs -> local L-dofs: the marker prolongated from the owners (MFEM's P)
    std::vector<int32_t> EssentialLDofs(const Array<int> &tlist) const
    {
        const int nt = fes_->GetTrueVSize();
        std::vector<double> mt((size_t)nt, 0.0), ml((size_t)height, 0.0);
        for (int i = 0; i < tlist.Size(); ++i) {
            if (tlist[i] < 0 || tlist[i] >= nt) throw std::invalid_argument("essential true dof out of range");
            mt[(size_t)tlist[i]] = 1.0;
        }
        fes_->Space().Prolongate(mt.data(), ml.data());
        std::vector<int32_t> out;
        for (int i = 0; i < height; ++i)
            if (ml[(size_t)i] != 0.0) out.push_back(i);
        return out;
    }
    void Setup()
    {
        const int dim = fes_->GetMesh()->Dimension(), ne = fes_->GetNE(), ns = dim * (dim + 1) / 2;
        unsigned kinds = 0;
        double kappa = 0.0, mass = 0.0, alpha = 1.0, conv[3] = {0, 0, 0};
        std::vector<double> kq, kmq, mq, cq;
        // every integrator samples its coefficient at the points of its own rule (on simplices
        // MFEM's GetRule differs per integrator; on quads / hexes the three rules coincide)
        std::map<int, std::pair<std::vector<double>, int>> pts;
        auto points = [&](int rule) -> const std::pair<std::vector<double>, int> & {
            auto it = pts.find(rule);
            if (it == pts.end()) {
                int n = 0;
                std::vector<double> x = dev_->Points(rule, dim, ne, n);  // a copy: Upload() may follow
                it = pts.emplace(rule, std::make_pair(std::move(x), n)).first;
            }
            return it->second;
        };
        auto accumulate = [&](Coefficient *q, double &cst, std::vector<double> &arr, int rule) {
            if (!q) {
                cst += 1.0;  // MassIntegrator() / DiffusionIntegrator(): coefficient 1
                if (!arr.empty())
                    for (double &v : arr) v += 1.0;
                return;
            }
            if (auto *c = dynamic_cast<ConstantCoefficient *>(q)) {
                cst += c->constant;
                if (!arr.empty())
                    for (double &v : arr) v += c->constant;
                return;
            }
            const auto &P = points(rule);
            std::vector<double> s = Sample(*q, P.first, dim, P.second);
            if (arr.empty()) arr.assign(s.size(), cst);
            for (size_t i = 0; i < s.size(); ++i) arr[i] += s[i];
        };
        for (auto &bi : integs_) {
            kinds |= bi->Kind();
            if (auto *d = dynamic_cast<DiffusionIntegrator *>(bi.get())) {
                if (!d->MQ_) {
                    accumulate(d->Q_, kappa, kq, CDFEM_RULE_DIFFUSION);
                    continue;
                }
                // MatrixCoefficient: symmetric tensor per point, xx,xy,(xz),yy,(yz),zz
                const std::vector<double> &P = points(CDFEM_RULE_DIFFUSION).first;
                const int nq = points(CDFEM_RULE_DIFFUSION).second;
                if (kmq.empty()) kmq.assign(P.size() / dim * ns, 0.0);
                ElementTransformation T;
                IntegrationPoint ip;
                DenseMatrix K;
                for (size_t i = 0; i < P.size() / dim; ++i) {
                    T.ElementNo = (int)(i / nq);
                    T.SetPoint(dim, &P[i * dim]);
                    d->MQ_->Eval(K, T, ip);
                    if (K.Height() != dim || K.Width() != dim)
                        throw std::invalid_argument("MatrixCoefficient: dim x dim values expected");
                    for (int a = 0, m = 0; a < dim; ++a)
                        for (int c = a; c < dim; ++c, ++m) {
                            const double sc = std::max(std::fabs(K(a, c)), std::fabs(K(c, a)));
                            if (std::fabs(K(a, c) - K(c, a)) > 1e-12 * std::max(sc, 1e-300))
                                throw std::invalid_argument("DiffusionIntegrator: only symmetric MatrixCoefficient values");
                            kmq[i * ns + m] += K(a, c);
                        }
                }
            } else if (auto *m = dynamic_cast<MassIntegrator *>(bi.get())) {
                accumulate(m->Q_, mass, mq, CDFEM_RULE_MASS);
            } else if (auto *c = dynamic_cast<ConvectionIntegrator *>(bi.get())) {
                if (auto *vc = dynamic_cast<VectorConstantCoefficient *>(c->Q_); vc && cq.empty()) {
                    for (int k = 0; k < dim; ++k) conv[k] += c->alpha * vc->GetVec()[k];
                } else {
                    const std::vector<double> &P = points(CDFEM_RULE_CONVECTION).first;
                    const int nq = points(CDFEM_RULE_CONVECTION).second;
                    if (cq.empty()) {
                        cq.resize(P.size());
                        for (size_t i = 0; i < P.size(); ++i) cq[i] = conv[i % dim];
                    }
                    ElementTransformation T;
                    IntegrationPoint ip;
                    Vector V;
                    for (size_t i = 0; i < P.size() / dim; ++i) {
                        T.ElementNo = (int)(i / nq);
                        T.SetPoint(dim, &P[i * dim]);
                        c->Q_->Eval(V, T, ip);
                        for (int k = 0; k < dim; ++k) cq[i * dim + k] += c->alpha * V[k];
                    }
                }
            }
        }
        const cdfem_form_coeffs f{kinds, kappa, kq.empty() ? nullptr : kq.data(), kmq.empty() ? nullptr : kmq.data(),
                                  alpha, conv, cq.empty() ? nullptr : cq.data(), mass, mq.empty() ? nullptr : mq.data()};
        // hexes / quads: partial assembly, or full assembly when SetAssemblyLevel asked for it; simplices: full
        // assembly (CSR on the GPU)
        if (dev_->Simplex() || Assembled()) check(cdfem_fa_setup_form(ctx(), &f), ctx(), "cdfem_fa_setup_form");
        else check(cdfem_pa_setup_form(ctx(), &f), ctx(), "cdfem_pa_setup_form");
    }

    FiniteElementSpace *fes_;
    std::vector<std::unique_ptr<BilinearFormIntegrator>> integs_;
    std::unique_ptr<DeviceSpace> dev_;
    std::unique_ptr<ConstrainedPAOperator> cop_;
    Vector XL_, BL_;  // FormLinearSystem's L-vectors, in HBM
    AssemblyLevel level_ = AssemblyLevel::PARTIAL;
    bool level_set_ = false;
};
using ParBilinearForm = BilinearForm;

inline void ConstrainedPAOperator::Mult(const Vector &x, Vector &y) const
{
    if (x.Size() != height) throw std::invalid_argument("HypreParMatrix::Mult: size");
    const int nl = a_->FESpace()->GetVSize(), off = (int)a_->FESpace()->FirstOwned();
    // one rank: P is the identity (on several ranks P is an exchange every rank joins, even one that
    // owns all its dofs)
    if (a_->FESpace()->NRanks() == 1) {
        y.SetSize(height);
        check(cdfem_pa_mult(a_->ctx(), x.Read(), y.Write(), 1, CDFEM_DEVICE), a_->ctx(), "cdfem_pa_mult");
        check(cdfem_synchronize(a_->ctx()), a_->ctx(), "cdfem_synchronize");
        return;
    }
    Vector xl(nl), yl(nl);
    a_->DeviceCtx().Prolongate(x, xl);
    check(cdfem_pa_mult(a_->ctx(), xl.Read(), yl.Write(), 1, CDFEM_DEVICE), a_->ctx(), "cdfem_pa_mult");
    check(cdfem_synchronize(a_->ctx()), a_->ctx(), "cdfem_synchronize");
    y.SetSubVectorOf(yl, off, height);
}

// ---- linear form ----------------------------------------------------------------------------------
class LinearFormIntegrator {
public:
    virtual ~LinearFormIntegrator() = default;
};
class DomainLFIntegrator : public LinearFormIntegrator {
public:
    explicit DomainLFIntegrator(Coefficient &f) : Q(&f) {}
    Coefficient *Q;
};

// b_i = (f, phi_i) over this rank's elements: a partial L-vector (ParLinearForm::Assemble)
class LinearForm : public Vector {
public:
    explicit LinearForm(FiniteElementSpace *f) : Vector(f->GetVSize()), fes_(f) {}
    void AddDomainIntegrator(LinearFormIntegrator *lfi) { integs_.emplace_back(lfi); }
    void Assemble()
    {
        DeviceSpace &dev = fes_->Space();
        const int dim = fes_->GetMesh()->Dimension();
        int nq = 0;
        const std::vector<double> &xyz = dev.Points(CDFEM_RULE_LINEARFORM, dim, fes_->GetNE(), nq);
        Vector fq((int)(xyz.size() / dim));
        double *f = fq.HostWrite();
        std::fill(f, f + fq.Size(), 0.0);
        for (auto &li : integs_) {
            auto *d = dynamic_cast<DomainLFIntegrator *>(li.get());
            if (!d) throw std::invalid_argument("LinearForm: only DomainLFIntegrator is supported");
            const std::vector<double> s = Sample(*d->Q, xyz, dim, nq);
            for (size_t i = 0; i < s.size(); ++i) f[i] += s[i];
        }
        // the point values cross PCIe (host Coefficient::Eval); the assembled vector stays in HBM
        check(cdfem_lf_assemble(dev.ctx(), fq.Read(), Write(), CDFEM_DEVICE), dev.ctx(), "cdfem_lf_assemble");
    }

private:
    FiniteElementSpace *fes_;
    std::vector<std::unique_ptr<LinearFormIntegrator>> integs_;
};
using ParLinearForm = LinearForm;

// ---- grid function ----------------------------------------------------------------------------
namespace detail {
// GLL nodes on [0,1] (H1 default basis, GaussLobatto) and the Lagrange basis through them
inline std::vector<double> gll_nodes(int p)
{
    // interior nodes = roots of P_p'; Newton with (1-t^2) P_p' = p (P_{p-1} - t P_p) and the
    // Legendre equation (1-t^2) P_p'' = 2 t P_p' - p (p+1) P_p
    std::vector<double> x((size_t)p + 1);
    x[0] = 0.0;
    x[(size_t)p] = 1.0;
    for (int i = 1; i < p; ++i) {
        double t = -std::cos(M_PI * i / p);
        for (int it = 0; it < 100; ++it) {
            double P0 = 1.0, P1 = t;
            for (int k = 2; k <= p; ++k) {
                const double P2 = ((2 * k - 1) * t * P1 - (k - 1) * P0) / k;
                P0 = P1;
                P1 = P2;
            }
            const double dP = p * (P0 - t * P1) / (1.0 - t * t);
            const double d2P = (2.0 * t * dP - p * (p + 1.0) * P1) / (1.0 - t * t);
            const double dt = dP / d2P;
            t -= dt;
            if (std::fabs(dt) < 1e-16) break;
        }
        x[(size_t)i] = 0.5 * (t + 1.0);
    }
    return x;
}
inline double lagrange(const std::vector<double> &nodes, int i, double t)
{
    double v = 1.0;
    for (size_t k = 0; k < nodes.size(); ++k)
        if ((int)k != i) v *= (t - nodes[k]) / (nodes[(size_t)i] - nodes[k]);
    return v;
}
inline void gauss_legendre01(int n, std::vector<double> &x, std::vector<double> &w)
{
    x.resize((size_t)n);
    w.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        double t = std::cos(M_PI * (i + 0.75) / (n + 0.5)), dP = 1.0;
        for (int it = 0; it < 100; ++it) {
            double P0 = 1.0, P1 = t;
            for (int k = 2; k <= n; ++k) {
                const double P2 = ((2 * k - 1) * t * P1 - (k - 1) * P0) / k;
                P0 = P1;
                P1 = P2;
            }
            dP = n * (t * P1 - P0) / (t * t - 1.0);
            const double dt = P1 / dP;
            t -= dt;
            if (std::fabs(dt) < 1e-16) break;
        }
        x[(size_t)i] = 0.5 * (1.0 - t);
        w[(size_t)i] = 1.0 / ((1.0 - t * t) * dP * dP);  // (2 / ((1-t^2) P'^2)) / 2
    }
}
}  // namespace detail

class GridFunction : public Vector {
public:
    explicit GridFunction(FiniteElementSpace *f) : Vector(f->GetVSize()), fes_(f) {}
    GridFunction &operator=(double v)
    {
        Vector::operator=(v);
        return *this;
    }
    GridFunction &operator=(const Vector &v)
    {
        Vector::operator=(v);
        return *this;
    }
    FiniteElementSpace *FESpace() const { return fes_; }
    FiniteElementSpace *ParFESpace() const { return fes_; }

    // nodal interpolation (GLL nodal basis: dof value = coefficient at the node); local dofs
    void ProjectCoefficient(Coefficient &q) { Project(q, nullptr); }
    void ProjectBdrCoefficient(Coefficient &q, const Array<int> &attr) { Project(q, &attr); }

    // MFEM ParGridFunction::GetTrueDofs / SetFromTrueDofs (R and P)
    void GetTrueDofs(Vector &tv) const
    {
        tv.SetSubVectorOf(*this, (int)fes_->FirstOwned(), fes_->GetTrueVSize());
    }
    void SetFromTrueDofs(const Vector &tv) { fes_->Space().Prolongate(tv, *this); }

    // ||u_h - u||_L2 over all ranks; tensor elements: Gauss rule of order max(2, 2p+3) or irs[geom]
    double ComputeL2Error(Coefficient &exact, const IntegrationRule *irs[] = nullptr) const
    {
        return std::sqrt(detail::allreduce_sum(L2(&exact, nullptr, irs, false), fes_->Comm()));
    }
    // ||u_h - u||_Lp with an optional weight (p = 2; diffusion_mms_ale.cpp:924)
    double ComputeLpError(double p, Coefficient &exact, Coefficient *weight = nullptr,
                          const IntegrationRule *irs[] = nullptr) const
    {
        if (p != 2.0) throw std::invalid_argument("ComputeLpError: only p = 2");
        return std::sqrt(detail::allreduce_sum(L2(&exact, weight, irs, false), fes_->Comm()));
    }
    double ComputeL2Norm(Coefficient &exact, const IntegrationRule *irs[] = nullptr) const
    {
        return std::sqrt(detail::allreduce_sum(L2(&exact, nullptr, irs, true), fes_->Comm()));
    }

private:
    void Project(Coefficient &q, const Array<int> *attr)
    {
        const int dim = fes_->GetMesh()->Dimension();
        const std::vector<double> &X = fes_->DofCoordinates();
        ElementTransformation T;
        IntegrationPoint ip;
        for (int i = 0; i < Size(); ++i) {
            if (attr && !fes_->OnMarkedBoundary(i, *attr, dim)) continue;
            T.SetPoint(dim, &X[(size_t)i * dim]);
            (*this)[i] = q.Eval(T, ip);
        }
    }
    // simplices: MFEM's rule IntRules.Get(TRIANGLE / TETRAHEDRON, order), the order of irs[geom]
    // or max(2, 2p + 3) (cdfem_simplex_rule_order), with the product's nodal basis
    double L2Simplex(Coefficient *exact, Coefficient *weight, const IntegrationRule *irs[], bool exact_only) const
    {
        const int dim = fes_->GetMesh()->Dimension(), p = fes_->GetOrder(), nd = fes_->NumElementDofs();
        const int geom = dim == 3 ? Geometry::TETRAHEDRON : Geometry::TRIANGLE;
        const int order = (irs && irs[geom]) ? irs[geom]->GetOrder() : std::max(2, 2 * p + 3);
        const int nq = cdfem_simplex_rule_order(dim, order, nullptr, nullptr);
        std::vector<double> xi((size_t)nq * dim), w(nq), phi((size_t)nq * nd);
        cdfem_simplex_rule_order(dim, order, xi.data(), w.data());
        check(cdfem_simplex_basis(dim, p, nq, xi.data(), phi.data(), nullptr), nullptr, "cdfem_simplex_basis");
        const std::vector<double> &V = fes_->ElementVertices();
        const std::vector<int32_t> &D = fes_->ElementDofs();
        ElementTransformation T;
        IntegrationPoint ip;
        double err2 = 0.0;
        for (int e = 0; e < fes_->GetNE(); ++e) {
            const double *ev = &V[(size_t)e * (dim + 1) * dim];
            double J[3][3] = {};
            for (int k = 0; k < dim; ++k)
                for (int m = 0; m < dim; ++m) J[k][m] = ev[(m + 1) * dim + k] - ev[k];
            const double det = dim == 3 ? J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
                                              J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                                              J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0])
                                        : J[0][0] * J[1][1] - J[0][1] * J[1][0];
            for (int q = 0; q < nq; ++q) {
                double X[3] = {0, 0, 0};
                for (int k = 0; k < dim; ++k) {
                    X[k] = ev[k];
                    for (int m = 0; m < dim; ++m) X[k] += J[k][m] * xi[(size_t)q * dim + m];
                }
                double uh = 0.0;
                if (!exact_only)
                    for (int l = 0; l < nd; ++l) uh += phi[(size_t)q * nd + l] * (*this)[D[(size_t)e * nd + l]];
                T.ElementNo = e;
                T.SetPoint(dim, X);
                const double u = exact->Eval(T, ip);
                const double wt = weight ? weight->Eval(T, ip) : 1.0;
                err2 += w[q] * std::fabs(det) * wt * (uh - u) * (uh - u);
            }
        }
        return err2;
    }
    // this rank's sum of squares (the callers all-reduce it)
    double L2(Coefficient *exact, Coefficient *weight, const IntegrationRule *irs[], bool exact_only) const
    {
        if (fes_->Simplex()) return L2Simplex(exact, weight, irs, exact_only);
        const int dim = fes_->GetMesh()->Dimension(), p = fes_->GetOrder(), d1 = p + 1;
        const int geom = dim == 3 ? Geometry::CUBE : Geometry::SQUARE;
        const int order = (irs && irs[geom]) ? irs[geom]->GetOrder() : std::max(2, 2 * p + 3);
        const int nq1 = order / 2 + 1;
        std::vector<double> qx, qw;
        detail::gauss_legendre01(nq1, qx, qw);
        const std::vector<double> nodes = detail::gll_nodes(p);
        std::vector<double> B((size_t)nq1 * d1);
        for (int q = 0; q < nq1; ++q)
            for (int i = 0; i < d1; ++i) B[(size_t)q * d1 + i] = detail::lagrange(nodes, i, qx[(size_t)q]);
        const int nv = 1 << dim, nd = dim == 3 ? d1 * d1 * d1 : d1 * d1;
        const int nq = dim == 3 ? nq1 * nq1 * nq1 : nq1 * nq1;
        const std::vector<double> &V = fes_->ElementVertices();
        const std::vector<int32_t> &D = fes_->ElementDofs();
        ElementTransformation T;
        IntegrationPoint ip;
        double err2 = 0.0;
        for (int e = 0; e < fes_->GetNE(); ++e) {
            const double *ev = &V[(size_t)e * nv * dim];
            const int32_t *ed = &D[(size_t)e * nd];
            for (int q = 0; q < nq; ++q) {
                const int qi[3] = {q % nq1, (q / nq1) % nq1, q / (nq1 * nq1)};
                double r[3] = {0, 0, 0}, w = 1.0;
                for (int k = 0; k < dim; ++k) {
                    r[k] = qx[(size_t)qi[k]];
                    w *= qw[(size_t)qi[k]];
                }
                // multilinear map and its Jacobian
                double X[3] = {0, 0, 0}, J[3][3] = {};
                for (int v = 0; v < nv; ++v) {
                    double phi = 1.0, dphi[3] = {1, 1, 1};
                    for (int k = 0; k < dim; ++k) {
                        const int b = (v >> k) & 1;
                        const double f = b ? r[k] : 1.0 - r[k], df = b ? 1.0 : -1.0;
                        phi *= f;
                        for (int l = 0; l < dim; ++l) dphi[l] *= (l == k) ? df : f;
                    }
                    for (int k = 0; k < dim; ++k) {
                        X[k] += phi * ev[v * dim + k];
                        for (int l = 0; l < dim; ++l) J[k][l] += dphi[l] * ev[v * dim + k];
                    }
                }
                const double det = dim == 3 ? J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
                                                  J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                                                  J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0])
                                            : J[0][0] * J[1][1] - J[0][1] * J[1][0];
                double uh = 0.0;
                if (!exact_only)
                    for (int l = 0; l < nd; ++l) {
                        const int li[3] = {l % d1, (l / d1) % d1, l / (d1 * d1)};
                        double phi = 1.0;
                        for (int k = 0; k < dim; ++k) phi *= B[(size_t)qi[k] * d1 + li[k]];
                        uh += phi * (*this)[ed[l]];
                    }
                T.ElementNo = e;
                T.SetPoint(dim, X);
                const double u = exact->Eval(T, ip);
                const double wt = weight ? weight->Eval(T, ip) : 1.0;
                err2 += w * std::fabs(det) * wt * (uh - u) * (uh - u);
            }
        }
        return err2;
    }
    FiniteElementSpace *fes_;
};
using ParGridFunction = GridFunction;

// ||u||_L2 over the (parallel) mesh; the geometry is multilinear / affine, so a low-order space suffices
inline double ComputeGlobalLpNorm(double p, Coefficient &exact, Mesh &mesh, const IntegrationRule *irs[])
{
    if (p != 2.0) throw std::invalid_argument("ComputeGlobalLpNorm: only p = 2");
    H1_FECollection fec(1, mesh.Dimension());  // exact_only: the basis is not evaluated
    FiniteElementSpace fes(&mesh, &fec);
    GridFunction z(&fes);
    return z.ComputeL2Norm(exact, irs);
}

// ---- Krylov solvers ---------------------------------------------------------------------------
class Solver : public Operator {
public:
    using Operator::Operator;
    virtual void SetOperator(const Operator &op) = 0;
};

// MFEM's Jacobi smoother as a preconditioner marker: the solve uses the operator's exact PA / CSR
// diagonal (ess rows 1) on the device
class OperatorJacobiSmoother : public Solver {
public:
    OperatorJacobiSmoother() = default;
    void SetOperator(const Operator &) override {}
    void Mult(const Vector &, Vector &) const override
    {
        throw std::logic_error("OperatorJacobiSmoother is applied inside the device solver");
    }
};

// PETSc's PCILU (zero fill, natural ordering) as a preconditioner marker: "-pc_type bjacobi
// -sub_pc_type ilu" (Input/petsc_circle.opts:6-8; on several ranks one block per rank, the owned
// diagonal block of the global matrix), or "-pc_type ilu" on one rank.  Factored once per operator
// on the device (ilu_kernels.hip) and applied inside the device GMRES.
class ILUPreconditioner : public Solver {
public:
    ILUPreconditioner() = default;
    void SetOperator(const Operator &) override {}
    void Mult(const Vector &, Vector &) const override
    {
        throw std::logic_error("ILUPreconditioner is applied inside the device solver");
    }
};

class IterativeSolver : public Solver {
public:
    IterativeSolver() = default;
    explicit IterativeSolver(MPI_Comm) {}
    void SetRelTol(double r) { rel_tol = r; }
    void SetAbsTol(double a) { abs_tol = a; }
    void SetMaxIter(int m) { max_iter = m; }
    void SetPrintLevel(int l) { print_level = l; }
    void SetOperator(const Operator &op) override
    {
        oper = dynamic_cast<const ConstrainedPAOperator *>(&op);
        if (!oper) throw std::invalid_argument("solver operator must come from BilinearForm::FormLinearSystem");
        height = width = op.Height();
    }
    void SetPreconditioner(Solver &pc)
    {
        pc_kind = dynamic_cast<OperatorJacobiSmoother *>(&pc) ? CDFEM_PC_JACOBI
                : dynamic_cast<ILUPreconditioner *>(&pc)     ? CDFEM_PC_ILU
                                                              : CDFEM_PC_NONE;
    }
    bool GetConverged() const { return converged; }
    int GetNumIterations() const { return final_iter; }
    double GetFinalNorm() const { return final_norm; }
    double GetSolveSeconds() const { return seconds; }

protected:
    // b, x: true-dof vectors; the device solve runs on the rank-local L-vectors (b prolongated)
    void Run(int method, int restart, const Vector &b, Vector &x) const
    {
        if (!oper) throw std::logic_error("SetOperator was not called");
        if (b.Size() != height) throw std::invalid_argument("solver Mult: size");
        cdfem_solver_params prm{};
        prm.method = method;
        prm.pc = pc_kind;
        prm.max_iter = max_iter;
        prm.restart = restart;
        prm.rel_tol = rel_tol;
        prm.abs_tol = abs_tol;
        prm.check_every = 0;
        prm.print_level = print_level;
        cdfem_solver_result res{};
        const BilinearForm *a = oper->Form();
        const int nl = a->FESpace()->GetVSize(), off = (int)a->FESpace()->FirstOwned();
        cdfem_ctx *c = a->ctx();
        int rc;
        if (a->FESpace()->NRanks() == 1 && &b != &x) {  // one rank: P is the identity (see ConstrainedPAOperator::Mult)
            x.SetSize(height);
            rc = cdfem_solve(c, &prm, b.Read(), x.Write(), CDFEM_DEVICE, &res);
        } else {
            bl_.SetSize(nl);
            xl_.SetSize(nl);
            a->DeviceCtx().Prolongate(b, bl_);
            rc = cdfem_solve(c, &prm, bl_.Read(), xl_.Write(), CDFEM_DEVICE, &res);
            if (rc == CDFEM_OK || rc == CDFEM_ERR_NOT_CONVERGED) x.SetSubVectorOf(xl_, off, height);
        }
        if (rc != CDFEM_OK && rc != CDFEM_ERR_NOT_CONVERGED) check(rc, c, "cdfem_solve");
        converged = res.converged != 0;
        final_iter = res.iterations;
        final_norm = res.final_norm;
        seconds = res.seconds;
        if (print_level > 0 && Mpi::Root())
            std::printf("   Iterations: %d  final norm: %.6e  (initial %.6e)  %s\n", final_iter, final_norm,
                        res.initial_norm, converged ? "converged" : "NOT converged");
    }
    const ConstrainedPAOperator *oper = nullptr;
    mutable Vector bl_, xl_;  // the solve's L-vectors, in HBM
    double rel_tol = 0.0, abs_tol = 0.0;
    int max_iter = 10, print_level = -1;
    int pc_kind = CDFEM_PC_NONE;
    mutable bool converged = false;
    mutable int final_iter = 0;
    mutable double final_norm = 0.0, seconds = 0.0;
};

// MFEM CGSolver semantics (mesh_recession_handler.cpp:270-276): (r,z) <= max(nom0 rel^2, abs^2).
// MFEM's tolerances are on the norm; cdfem_solve takes them as norms too.
class CGSolver : public IterativeSolver {
public:
    using IterativeSolver::IterativeSolver;
    void Mult(const Vector &b, Vector &x) const override { Run(CDFEM_CG, 0, b, x); }
};

// GMRES with PETSc KSPGMRES semantics (left preconditioning, classical Gram-Schmidt)
class GMRESSolver : public IterativeSolver {
public:
    using IterativeSolver::IterativeSolver;
    void SetKDim(int m) { kdim = m; }
    void Mult(const Vector &b, Vector &x) const override { Run(CDFEM_GMRES, kdim, b, x); }

private:
    int kdim = 30;
};

// BiCGStab with PETSc KSPBCGS semantics (left preconditioning, ||M^-1 r|| <= max(rtol ||M^-1 b||, atol));
// not MFEM's BiCGSTABSolver, whose stopping rules differ
class PetscBCGSSolver : public IterativeSolver {
public:
    using IterativeSolver::IterativeSolver;
    void Mult(const Vector &b, Vector &x) const override { Run(CDFEM_BICGSTAB, 0, b, x); }
};

// ---- PETSc-named front end (linear_convection_diffusion_2D.cpp:268-282, :364-375) --------------
// MFEMInitializePetsc reads an options file with the keys the reference's Input/*.opts set:
// -ksp_type {gmres, cg, bcgs}, -ksp_rtol, -ksp_atol, -ksp_max_it, -ksp_gmres_restart, -pc_type
// {jacobi, none, ilu, bjacobi with -sub_ksp_type preonly -sub_pc_type ilu}.  A solver with an options
// prefix reads "-<prefix><key>" (Input/petsc_nonlinear.opts: -newton_ls_ksp_rtol ...).  Absent keys
// take PETSc's defaults: gmres, restart 30, rtol 1e-5, atol 1e-50, max_it 10000, and PETSc's default
// preconditioner, ILU(0) for an assembled matrix on one rank; where that is not available (matrix-
// free operators, several ranks, where PETSc would use block Jacobi) Jacobi is used and a note printed.
// -ksp_type cg follows MFEM CGSolver's stopping test (sqrt(r.z)); PETSc's KSPCG default tests the
// preconditioned residual norm ||M^-1 r|| instead, so iteration counts can differ by a few.
struct PetscOptionsStore {
    std::map<std::string, std::string> kv;
    std::string Get(const std::string &k, const std::string &def) const
    {
        auto it = kv.find(k);
        return it == kv.end() ? def : it->second;
    }
    bool Has(const std::string &k) const { return kv.count(k) != 0; }
};
inline PetscOptionsStore &PetscOptions()
{
    static PetscOptionsStore s;
    return s;
}

inline void MFEMInitializePetsc(int * = nullptr, char *** = nullptr, const char *rc_file = nullptr,
                                const char * = nullptr)
{
    if (!rc_file) return;
    std::ifstream in(rc_file);
    if (!in) throw std::runtime_error(std::string("cannot open PETSc options file ") + rc_file);
    std::string line;
    while (std::getline(in, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        std::istringstream ss(line);
        std::string key, val;
        if (!(ss >> key)) continue;
        ss >> val;
        PetscOptions().kv[key] = val;
    }
}
inline void MFEMFinalizePetsc() {}

// The drivers' options-file choice (not MFEM API; the drivers' "-opts" argument):
//  * an options file that exists is read (MFEMInitializePetsc);
//  * an explicitly given file that does not exist: the reference's warning ("PETSc options file not
//    found: ... Proceeding without options file.", linear_convection_diffusion_1D.cpp:310-324) and
//    PETSc's defaults;
//  * no -opts and no Input/petsc.opts in the working directory (the reference's default path, which
//    exists beside the reference drivers): the values of the reference's Input/petsc.opts:2-6
//    (gmres, rtol 1e-10, atol 1e-12, max_it 500, jacobi), so a run from any directory solves as the
//    reference's default run does.
// Returns the file to pass to MFEMInitializePetsc (nullptr: none).
inline const char *DriverPetscOptionsFile(const std::string &given, const char *default_path = "Input/petsc.opts")
{
    static std::string chosen;
    if (!given.empty()) {
        if (std::ifstream(given).good()) return (chosen = given).c_str();
        if (Mpi::Root())
            std::cerr << "PETSc options file not found: " << given << ". Proceeding without options file." << std::endl;
        return nullptr;
    }
    if (std::ifstream(default_path).good()) return (chosen = default_path).c_str();
    auto &o = PetscOptions().kv;
    o.emplace("-ksp_type", "gmres");
    o.emplace("-ksp_rtol", "1.0e-10");
    o.emplace("-ksp_atol", "1.0e-12");
    o.emplace("-ksp_max_it", "500");
    o.emplace("-pc_type", "jacobi");
    return nullptr;
}

class PetscParMatrix : public Operator {
public:
    // PetscParMatrix(MPI_COMM_WORLD, A_true, Operator::PETSC_MATAIJ)  (:367)
    PetscParMatrix(MPI_Comm comm, const Operator *A, Operator::Type = PETSC_MATAIJ)
        : Operator(A->Height(), A->Width()), A_(A), comm_(comm) {}
    // PetscParMatrix(A_hyp, Operator::PETSC_MATAIJ)  (diffusion_mms.cpp:449)
    explicit PetscParMatrix(const HypreParMatrix *A, Operator::Type = PETSC_MATAIJ)
        : Operator(A->Height(), A->Width()), A_(A) {}
    void Mult(const Vector &x, Vector &y) const override { A_->Mult(x, y); }
    const Operator *Inner() const { return A_; }
    MPI_Comm GetComm() const { return comm_; }

private:
    const Operator *A_;
    MPI_Comm comm_ = MPI_COMM_WORLD;
};

class PetscLinearSolver : public Solver {
public:
    explicit PetscLinearSolver(MPI_Comm, const std::string &prefix = std::string(), bool = true, bool = false)
        : prefix_(prefix) {}
    explicit PetscLinearSolver(const PetscParMatrix &A, const std::string &prefix = std::string(), bool = false)
        : prefix_(prefix)
    {
        SetOperator(A);
    }
    void SetOperator(const Operator &op) override
    {
        const auto *pm = dynamic_cast<const PetscParMatrix *>(&op);
        const Operator &inner = pm ? *pm->Inner() : op;
        const auto *cop = dynamic_cast<const ConstrainedPAOperator *>(&inner);
        if (!cop) throw std::invalid_argument("PetscLinearSolver: operator must come from FormLinearSystem");
        Configure(*cop);
        solver_->SetOperator(inner);
        height = width = op.Height();
    }
    void SetRelTol(double r) { rel_ = r; if (solver_) solver_->SetRelTol(r); }
    void SetAbsTol(double a) { abs_ = a; if (solver_) solver_->SetAbsTol(a); }
    void SetMaxIter(int m) { maxit_ = m; if (solver_) solver_->SetMaxIter(m); }
    void SetPrintLevel(int l) { print_ = l; if (solver_) solver_->SetPrintLevel(l); }
    void Mult(const Vector &b, Vector &x) const override
    {
        if (!solver_) throw std::logic_error("PetscLinearSolver: no operator");
        solver_->Mult(b, x);
    }
    bool GetConverged() const { return solver_ && solver_->GetConverged(); }
    int GetNumIterations() const { return solver_ ? solver_->GetNumIterations() : 0; }
    double GetFinalNorm() const { return solver_ ? solver_->GetFinalNorm() : 0.0; }
    double GetSolveSeconds() const { return solver_ ? solver_->GetSolveSeconds() : 0.0; }

private:
    std::string Opt(const std::string &key, const std::string &def) const
    {
        return PetscOptions().Get("-" + prefix_ + key, def);
    }
    void Configure(const ConstrainedPAOperator &cop)
    {
        const std::string type = Opt("ksp_type", "gmres");
        if (type == "cg") solver_ = std::make_unique<CGSolver>();
        else if (type == "gmres") {
            auto g = std::make_unique<GMRESSolver>();
            g->SetKDim(std::stoi(Opt("ksp_gmres_restart", "30")));
            solver_ = std::move(g);
        } else if (type == "bcgs")
            solver_ = std::make_unique<PetscBCGSSolver>();
        else
            throw std::invalid_argument("unsupported -" + prefix_ + "ksp_type " + type);
        solver_->SetRelTol(rel_ >= 0 ? rel_ : std::stod(Opt("ksp_rtol", "1e-5")));
        solver_->SetAbsTol(abs_ >= 0 ? abs_ : std::stod(Opt("ksp_atol", "1e-50")));
        solver_->SetMaxIter(maxit_ >= 0 ? maxit_ : std::stoi(Opt("ksp_max_it", "10000")));
        solver_->SetPrintLevel(print_);
        const FiniteElementSpace *fes = cop.Form()->FESpace();
        // assembled: a simplex space (one rank, or a general partition), or a quad / hex form at LEGACY / FULL
        const bool ilu_ok = fes->Simplex() || cop.Form()->Assembled();
        std::string pc = Opt("pc_type", "");
        if (pc.empty()) {  // PETSc's default preconditioner: ILU on one rank, block Jacobi + ILU on several
            pc = ilu_ok ? (fes->NRanks() == 1 ? "ilu" : "bjacobi") : "jacobi";
            if (!ilu_ok && Mpi::Root())
                std::fprintf(stderr, "note: no -%spc_type: PETSc's default ILU / block Jacobi is not available for this "
                                     "(matrix-free) operator; using Jacobi\n", prefix_.c_str());
        }
        if (pc == "jacobi") {
            solver_->SetPreconditioner(jac_);
        } else if (pc == "ilu" || pc == "bjacobi") {
            // block Jacobi: one block per rank (the owned diagonal block of the global matrix),
            // solved by its sub-PC (preonly + ILU(0)); on one rank that is PCILU itself.  PETSc's
            // PCILU has no parallel (MPIAIJ) factorisation, so -pc_type ilu needs one rank.
            const std::string sub = pc == "ilu" ? "ilu" : Opt("sub_pc_type", "ilu");
            const std::string subksp = Opt("sub_ksp_type", "preonly");
            if (sub != "ilu" || subksp != "preonly")
                throw std::invalid_argument("unsupported block-Jacobi sub solver " + subksp + "/" + sub);
            if (pc == "ilu" && fes->NRanks() > 1)
                throw std::invalid_argument("-pc_type ilu on several ranks (PETSc has no parallel ILU; use bjacobi)");
            if (!ilu_ok) throw std::invalid_argument("-pc_type " + pc + " needs an assembled operator (a simplex mesh, or "
                                                "SetAssemblyLevel(AssemblyLevel::LEGACY) on quads / hexes)");
            solver_->SetPreconditioner(ilu_);
        } else if (pc != "none") {
            throw std::invalid_argument("unsupported -" + prefix_ + "pc_type " + pc);
        }
    }
    std::string prefix_;
    std::unique_ptr<IterativeSolver> solver_;
    OperatorJacobiSmoother jac_;
    ILUPreconditioner ilu_;
    double rel_ = -1.0, abs_ = -1.0;
    int maxit_ = -1, print_ = -1;
};

// ParaView output is outside the hot path: the collection accepts the reference's
// set-up calls (:423-430) so the driver text compiles, and Save() reports that it is not provided.
enum class VTKFormat { ASCII, BINARY, BINARY32 };
class ParaViewDataCollection {
public:
    ParaViewDataCollection(const std::string &name, Mesh *) : name_(name) {}
    void SetPrefixPath(const std::string &) {}
    void SetLevelsOfDetail(int) {}
    void SetDataFormat(VTKFormat) {}
    void SetHighOrderOutput(bool) {}
    void RegisterField(const std::string &, GridFunction *) {}
    void SetCycle(int) {}
    void SetTime(double) {}
    void Save() { throw std::runtime_error("ParaView output (" + name_ + ") is not provided by this build"); }

private:
    std::string name_;
};

}  // namespace mfem
}  // namespace cdfem
