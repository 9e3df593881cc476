// host_util.hpp — host-side utilities of the library: the typed errors and their mapping to the C-ABI's
// return codes, checked HIP calls, device allocation, and the profiling marks.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <stdexcept>
#include <string>

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

template <typename T>
void dfree(T *&p)
{
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}

template <typename T>
T *dalloc(size_t n)
{
    void *p = nullptr;
    if (n == 0) n = 1;
    HIPCHK(hipMalloc(&p, n * sizeof(T)));
    return static_cast<T *>(p);
}

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
