// krylov_host.hpp — what the GMRES and BiCGStab drivers and launchers share on the host and that needs no
// HIP: the entries-per-thread rule of the vector kernels, the lag-one host poll, and the first-use allocation
// of a solver's state.  Plain C++ (tests/cpp/krylov_host_check.cpp builds it with g++); included by
// cdfem_internal.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "dispatch.hpp"
#include "handles.hpp"

namespace cdfem {

constexpr int kRedThreads = 256;  // threads per block of the reduction and vector kernels (reduce.hpp)

// ---- entries per thread (EPT) of the vector kernels ----------------------------------------------
// The smallest of 4, 5, 6, 8 whose grid is resident in one round, blocks <= resident(E) (CUs x resident
// blocks per CU), so no tail of a few blocks runs a second round alone; 8 when none is.  (C2: n = 129^3 is
// 2097 blocks of 1024 entries against 2048 resident slots at EPT 4, 1678 at EPT 5.)  A function of the vector
// size and the device alone, so a size's sums always run in the same order.
template <class Resident>
int pick_ept(int64_t n, Resident &&resident)
{
    for (int e : {4, 5, 6}) {
        const int64_t chunk = (int64_t)kRedThreads * e;
        if ((n + chunk - 1) / chunk <= (int64_t)resident(e)) return e;
    }
    return 8;
}

// the choice, kept for vectors of n entries (one per solver in the context)
struct EptCache {
    int ept = 4;
    int64_t n = -1;
};
template <class Resident>
int cached_ept(EptCache &cache, int64_t n, Resident &&resident)
{
    if (cache.n != n) cache = EptCache{pick_ept(n, resident), n};
    return cache.ept;
}

// f(EPT as a constant): 5, 6, 8, any other is 4
template <class F>
void with_ept(int ept, F &&f)
{
    const auto run = [&](auto E) {
        f(E);
        return true;
    };
    if (!dispatch_value<5, 6, 8>(ept, false, run)) run(std::integral_constant<int, 4>{});
}

// ---- the lag-one host poll -----------------------------------------------------------------------
// The host queues steps without waiting for the device.  The last scalar kernel of a polled step writes
// the head of the state into a pinned slot of its own (post_head, krylov_core.hpp), and the host marks
// the step's completion with an event: post n since reset() records event n & 1.  From the second post
// on, post() then waits for the PREVIOUS post's event and returns that post's slot: the host reads the
// state of exactly the step it waited for, never the current one's, with the next steps already queued,
// so the GPU never idles on the host.  The state is the same on every rank (all-reduced sums), so every
// rank leaves its loop at the same step and their collectives pair up.
//
// Work queued past a stop, for a post every k-th step: a stop at step s is posted by the first polled
// step q >= s, q <= s + k - 1, and read at the next post, after step q + k is queued.  So q + k - s steps,
// at most 2k - 1, are queued past the stop (fewer where the loop's own bound ends it: a GMRES cycle, a
// BiCGStab max_iter).  Their solver kernels exit at entry on the state's flag; their operator applies,
// which do not check, run.
//
// record(i) records event i on the stream, wait(i) blocks the host until event i has completed.
template <class Record, class Wait>
class LagPoll {
    Record record_;
    Wait wait_;
    int nposts_ = 0, prev_ = -1;

public:
    LagPoll(Record record, Wait wait) : record_(record), wait_(wait) {}
    void reset()
    {
        nposts_ = 0;
        prev_ = -1;
    }
    // the step just queued posts into slot (>= 0); returns the slot that may now be read, -1 on the first post
    int post(int slot)
    {
        record_(nposts_ & 1);
        const int prev = prev_;
        prev_ = slot;
        ++nposts_;
        if (prev < 0) return -1;
        wait_(nposts_ & 1);  // the previous post's event, (nposts - 2) & 1
        return prev;
    }
};

// ---- a solver's device state, pinned poll slots and the poll's two events, on first use ----------
template <class State, class Head>
void krylov_state_alloc(DevBuf<State> &st, PinBuf<Head> &poll, size_t slots, Event (&ev)[2])
{
    if (st) return;
    st.alloc(1);
    poll.alloc(slots);
    for (auto &e : ev) e.create(false);
}

}  // namespace cdfem
