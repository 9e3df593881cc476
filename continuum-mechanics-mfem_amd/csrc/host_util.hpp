// host_util.hpp — host-side utilities of the library: the typed errors and their mapping to the C-ABI's
// return codes, checked HIP calls, uploads into the owning buffers of handles.hpp, and the profiling marks.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "cdfem_internal.hpp"

namespace cdfem {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };
struct StateError : std::runtime_error { using std::runtime_error::runtime_error; };
struct UnsupportedError : std::runtime_error { using std::runtime_error::runtime_error; };

inline void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(x) ::cdfem::hip_check((x), #x)

template <typename F>
int guarded(cdfem_ctx *c, F &&f)
{
    if (!c) return CDFEM_ERR_ARG;
    try {
        c->err.clear();
        return f();
    } catch (const ArgError &e) {
        c->err = e.what();
        return CDFEM_ERR_ARG;
    } catch (const StateError &e) {
        c->err = e.what();
        return CDFEM_ERR_STATE;
    } catch (const UnsupportedError &e) {
        c->err = e.what();
        return CDFEM_ERR_UNSUPPORTED;
    } catch (const HipError &e) {
        c->err = e.what();
        return CDFEM_ERR_HIP;
    } catch (const std::bad_alloc &) {
        c->err = "host allocation failed";
        return CDFEM_ERR_HIP;
    } catch (const std::exception &e) {
        c->err = e.what();
        return CDFEM_ERR_ARG;
    }
}

// b <- n elements of host memory: allocated (what it held is freed first) and copied on the context stream.
// The source must stay alive until the stream has been synchronised.
template <typename T, typename Mem>
void upload(cdfem_ctx *c, Buf<T, Mem> &b, const T *src, size_t n)
{
    b.assign(src, n, [c](void *dst, const void *s, size_t bytes) {
        HIPCHK(hipMemcpyAsync(dst, s, bytes, hipMemcpyHostToDevice, c->stream));
    });
}
template <typename T, typename Mem>
void upload(cdfem_ctx *c, Buf<T, Mem> &b, const std::vector<T> &v)
{
    upload(c, b, v.data(), v.size());
}

// ---- call-order checks and copies of the entry points (capi.hip) -----------------------------------
void require_mesh(cdfem_ctx *c);       // StateError before a mesh upload
void require_pa(cdfem_ctx *c);         // ... before an operator setup
void require_partition(cdfem_ctx *c);  // several ranks: a declared partition
// a device pointer holding n doubles of src (staged through staging when src is on the host)
const double *dev_in(cdfem_ctx *c, const double *src, int where, double *staging, size_t n);
// dst (host: synchronous; device: unless it is dsrc itself) <- n doubles at dsrc
void dev_out(cdfem_ctx *c, double *dst, int where, const double *dsrc, size_t n);

// ---- profiling (capi.hip) -------------------------------------------------------------------------
void prof_mark(cdfem_ctx *c, int k, bool begin);
void prof_collect(cdfem_ctx *c);

// f() bracketed by kernel id k's begin and end marks: the first CDFEM_LAUNCH inside f takes the armed
// event pair.  (A function, not a scope guard: the end mark can throw.)
template <typename F>
void timed(cdfem_ctx *c, int k, F &&f)
{
    prof_mark(c, k, true);
    f();
    prof_mark(c, k, false);
}

}  // namespace cdfem
