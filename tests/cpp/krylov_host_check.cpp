// krylov_host_check.cpp — csrc/krylov_host.hpp on the host alone (tests/test_krylov_host.py): LagPoll driven
// over a fake in-order queue in the two shapes the drivers use, and pick_ept against a brute-force restatement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "krylov_host.hpp"

using namespace cdfem;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_case);    \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

static char g_case[128] = "";

// The fake queue.  Steps are queued in order and complete in order; step i posts "done iff i >= stop" into
// the slot it was given.  An event recorded after step i was queued completes when step i has.  Every record,
// wait and slot read is logged and checked where it happens.
struct FakeQueue {
    int stop = 0;
    int queued = 0;                 // steps queued so far: 0 .. queued - 1
    int completed = 0;              // steps the host knows to have completed (by a wait): 0 .. completed - 1
    struct Rec {
        int event, after;           // the event, and the number of steps queued when it was recorded
    };
    std::vector<Rec> records;       // in order
    int latest[2] = {-1, -1};       // per event: index of its latest record, -1 before the first
    std::vector<int> slot_step;     // per slot: the last queued step that posts into it, -1 none
    int waits = 0, reads = 0;

    explicit FakeQueue(int stop_, int slots) : stop(stop_), slot_step(slots, -1) {}

    void queue_step(int slot)  // slot < 0: the step posts nowhere
    {
        if (slot >= 0) slot_step[slot] = queued;
        ++queued;
    }
    void record(int e)
    {
        CHECK(e == 0 || e == 1);
        latest[e] = (int)records.size();
        records.push_back({e, queued});
    }
    // the wait of a lag-one post: for the record before the latest one, which must still be its event's latest
    void wait_lagged(int e)
    {
        CHECK(e == 0 || e == 1);
        CHECK(records.size() >= 2);
        CHECK(latest[e] == (int)records.size() - 2);  // recorded before, by the previous post, not re-recorded
        complete(e);
    }
    // a synchronous wait: for the record just made
    void wait_now(int e)
    {
        CHECK(latest[e] == (int)records.size() - 1);
        complete(e);
    }
    void complete(int e)
    {
        ++waits;
        const int upto = records[latest[e]].after;
        if (upto > completed) completed = upto;
    }
    // the host reads a slot: the step that posted it has completed, and no step queued since posts into it
    // (the device may run ahead of what the host has waited for), so what it reads is that step's state
    bool read_done(int slot, int expect_step)
    {
        ++reads;
        CHECK(slot >= 0 && slot < (int)slot_step.size());
        CHECK(slot_step[slot] == expect_step);
        CHECK(expect_step < completed);
        return expect_step >= stop;
    }
};

// ---- the BiCGStab shape: a post every k-th step into slot (i / k) % 4 ------------------------------
static void bicgstab_shape(int k, int s)
{
    std::snprintf(g_case, sizeof g_case, "bicgstab k=%d s=%d", k, s);
    constexpr int kSlots = 4, kMax = 200;
    FakeQueue q(s, kSlots);
    LagPoll lag([&](int e) { q.record(e); }, [&](int e) { q.wait_lagged(e); });
    int nposts = 0, prev_step = -1, prev_slot = -1, left_at = -1;
    for (int i = 0; i < kMax; ++i) {
        const bool polled = (i + 1) % k == 0;
        const int slot = (i / k) % kSlots;
        q.queue_step(polled ? slot : -1);
        if (!polled) continue;
        const size_t nrec = q.records.size();
        const int waits = q.waits;
        const int got = lag.post(slot);
        CHECK(q.records.size() == nrec + 1 && q.records.back().event == (nposts & 1));  // post n records event n & 1
        CHECK(got == prev_slot);                      // the previous post's slot, -1 on the first
        CHECK(q.waits == waits + (nposts > 0 ? 1 : 0));
        CHECK(got != slot);                           // never the current post's
        const int read_step = prev_step;
        prev_step = i;
        prev_slot = slot;
        ++nposts;
        if (got >= 0 && q.read_done(got, read_step)) {
            CHECK(read_step >= s);
            left_at = i;
            break;
        }
        CHECK(got < 0 || read_step < s);              // no later leave than the first such post
    }
    // q: the first polled step >= s; the loop leaves at the post of step q + k
    int first = k - 1;
    while (first < s) first += k;
    CHECK(left_at == first + k);
    const int past = q.queued - 1 - s;                // steps queued after step s
    CHECK(past == first + k - s);
    CHECK(past <= 2 * k - 1);
    CHECK(q.reads == nposts - 1);
}

// ---- the GMRES shape: cycles of m steps, a post every k-th step and on the cycle's last, slot = the step
// within the cycle, reset() at the cycle's end, then the synchronous check on event 0 ------------------
static void gmres_shape(int k, int s, int m)
{
    std::snprintf(g_case, sizeof g_case, "gmres k=%d s=%d m=%d", k, s, m);
    FakeQueue q(s, m);
    LagPoll lag([&](int e) { q.record(e); }, [&](int e) { q.wait_lagged(e); });
    const int stop_cycle = s / m, js = s % m;
    bool over = false;
    for (int cycle = 0; !over; ++cycle) {
        CHECK(cycle <= stop_cycle);
        int nposts = 0, prev_j = -1, left_at = -1;
        for (int j = 0; j < m; ++j) {
            const int g = cycle * m + j;              // the step's number over the solve
            const bool polled = j == m - 1 || (j + 1) % k == 0;
            q.queue_step(j);                          // every step posts into its own slot
            CHECK(g == q.queued - 1);
            if (!polled) continue;
            const int got = lag.post(j);
            CHECK(q.records.back().event == (nposts & 1));
            CHECK(got == prev_j && got != j);
            const int read_j = prev_j;
            prev_j = j;
            ++nposts;
            // the cycle is done at the stop step (and at its last step, whose post nothing in the loop reads)
            if (got >= 0 && q.read_done(got, cycle * m + read_j)) {
                CHECK(cycle * m + read_j >= s);
                left_at = j;
                break;
            }
            CHECK(got < 0 || cycle * m + read_j < s);
        }
        lag.reset();
        const int last = q.queued - 1;
        if (cycle == stop_cycle) {
            // q: the first polled step of the cycle >= js; the loop leaves at the next polled step after it,
            // q + k or the cycle's last, or runs out at the cycle's last step when q is that step
            int first = -1;
            for (int j = js; j < m && first < 0; ++j)
                if (j == m - 1 || (j + 1) % k == 0) first = j;
            const int end = first + k < m - 1 ? first + k : m - 1;
            CHECK(last == cycle * m + end);
            CHECK(left_at == (first == m - 1 ? -1 : end));
            const int past = last - s;
            CHECK(past == end - js && past <= first + k - js && past <= 2 * k - 1 && past <= m - 1 - js);
        } else {
            CHECK(left_at == -1 && last == cycle * m + m - 1);  // a cycle before the stop runs all its steps
        }
        // the cycle's end: slot 0 of the driver, synchronously on event 0 (the poll starts over after it)
        q.record(0);
        q.wait_now(0);
        CHECK(q.completed == q.queued);
        over = last >= s;
        CHECK(over == (cycle == stop_cycle));
    }
}

// ---- pick_ept against a restatement -----------------------------------------------------------------
template <class Resident>
static int brute_ept(int64_t n, Resident &&resident)
{
    const int cand[4] = {4, 5, 6, 8};
    for (int e : cand) {
        int64_t blocks = 0;
        for (int64_t covered = 0; covered < n; covered += 256 * e) ++blocks;  // (kRedThreads entries per e)
        if (blocks <= resident(e)) return e;
    }
    return 8;
}

static void ept_checks()
{
    static_assert(kRedThreads == 256);
    const int64_t sizes[] = {1, 1023, 1024, 1025, 4913, 35937, 2146689};
    const int64_t caps[] = {0, 1, 2, 4, 5, 6, 29, 36, 1398, 1677, 1678, 2047, 2048, 2097, 4096, 1 << 20};
    for (int64_t n : sizes) {
        for (int64_t cap : caps) {
            std::snprintf(g_case, sizeof g_case, "pick_ept n=%lld cap=%lld", (long long)n, (long long)cap);
            const auto constant = [&](int) { return cap; };
            CHECK(pick_ept(n, constant) == brute_ept(n, constant));
            // per E: fewer resident blocks the more entries a thread holds (registers), in two steps
            const auto per_e = [&](int e) { return e <= 4 ? cap : e <= 6 ? cap * 3 / 4 : cap / 2; };
            CHECK(pick_ept(n, per_e) == brute_ept(n, per_e));
            const auto rising = [&](int e) { return cap * e / 4; };
            CHECK(pick_ept(n, rising) == brute_ept(n, rising));
        }
    }
    // the rule's own example: 129^3 entries are 2,097 blocks at EPT 4 against 2,048 resident slots, 1,678 at 5
    std::snprintf(g_case, sizeof g_case, "pick_ept 129^3");
    CHECK((2146689 + 1023) / 1024 == 2097 && (2146689 + 1279) / 1280 == 1678);
    CHECK(pick_ept(2146689, [](int) { return 2048; }) == 5);
    CHECK(pick_ept(2146689, [](int) { return 2097; }) == 4);
    CHECK(pick_ept(2146689, [](int) { return 1; }) == 8);

    // the cache asks once per vector size; with_ept hands 5, 6, 8 on and takes any other for 4
    EptCache cache;
    int asked = 0;
    const auto counting = [&](int) { return ++asked, 2048; };
    CHECK(cached_ept(cache, 2146689, counting) == 5 && asked == 2);
    CHECK(cached_ept(cache, 2146689, counting) == 5 && asked == 2);
    CHECK(cached_ept(cache, 4913, counting) == 4 && asked == 3 && cache.n == 4913);
    for (int e = 0; e <= 9; ++e) {
        int got = -1;
        with_ept(e, [&](auto E) { got = E(); });
        CHECK(got == (e == 5 || e == 6 || e == 8 ? e : 4));
    }
}

int main()
{
    int cases = 0;
    for (int k = 1; k <= 8; ++k)
        for (int s = 0; s <= 40; ++s) {
            bicgstab_shape(k, s);
            ++cases;
            for (int m : {1, 5, 7, 30}) {
                gmres_shape(k, s, m);
                ++cases;
            }
        }
    ept_checks();
    std::printf("krylov host ok: %d poll cases\n", cases);
    return 0;
}
