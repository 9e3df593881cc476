// handles.hpp — move-only owners of the context's raw resources: device buffers, pinned host buffers and
// events.  No HIP header: the resources are reached through six functions that are only declared here.
// The library defines them over the HIP runtime (capi.hip), the host check over malloc
// (tests/cpp/ctx_state_check.cpp).  A handle converts implicitly to its raw pointer, so kernel arguments,
// pointer arithmetic, null tests and the HIP calls read as they do on a raw pointer; only a function
// template that takes its arguments by value (hipExtLaunchKernelGGL, CDFEM_LAUNCH) needs .get(), and says so
// at compile time (the copy is deleted).
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

struct ihipEvent_t;  // what hipEvent_t points to

namespace cdfem {

// acquire: throws HipError (host_util.hpp) on failure; release: noexcept, never called with null
void *raw_device_alloc(size_t bytes);
void raw_device_free(void *p) noexcept;
void *raw_pinned_alloc(size_t bytes);
void raw_pinned_free(void *p) noexcept;
ihipEvent_t *raw_event_create(bool timing);
void raw_event_destroy(ihipEvent_t *e) noexcept;

struct DeviceMem {
    static void *alloc(size_t bytes) { return raw_device_alloc(bytes); }
    static void free(void *p) noexcept { raw_device_free(p); }
};
struct PinnedMem {
    static void *alloc(size_t bytes) { return raw_pinned_alloc(bytes); }
    static void free(void *p) noexcept { raw_pinned_free(p); }
};

// n elements of T in Mem's memory; null until alloc / assign
template <typename T, typename Mem>
class Buf {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~Buf() { reset(); }

    void reset() noexcept
    {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // frees what it held first; n == 0 allocates one element (a non-null pointer of size() 0)
    void alloc(size_t n)
    {
        reset();
        p_ = static_cast<T *>(Mem::alloc((n ? n : 1) * sizeof(T)));
        n_ = n;
    }
    // alloc(n), then copy(dst, src, bytes) unless n == 0
    template <typename Copy>
    void assign(const T *src, size_t n, Copy &&copy)
    {
        alloc(n);
        if (n) copy(static_cast<void *>(p_), static_cast<const void *>(src), n * sizeof(T));
    }
    template <typename Copy>
    void assign(const std::vector<T> &v, Copy &&copy) { assign(v.data(), v.size(), copy); }

    size_t size() const { return n_; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
};
template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using PinBuf = Buf<T, PinnedMem>;

class Event {
    ihipEvent_t *e_ = nullptr;

public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }

    void reset() noexcept
    {
        if (e_) raw_event_destroy(e_);
        e_ = nullptr;
    }
    void create(bool timing)
    {
        reset();
        e_ = raw_event_create(timing);
    }
    ihipEvent_t *get() const { return e_; }
    operator ihipEvent_t *() const { return e_; }
};

}  // namespace cdfem
