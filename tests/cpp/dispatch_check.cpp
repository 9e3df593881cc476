// csrc/dispatch.hpp on its own (no HIP): every listed value reaches the lambda as exactly that constant, bools
// arrive in the order written, and a value outside the list gives the fallback without a call.
#include <cstdio>
#include <type_traits>

#include "dispatch.hpp"

using namespace cdfem;

static int fails = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

enum Err { Ok = 0, Invalid = 1 };

int main()
{
    // every listed value: the lambda runs once, with that constant, typed as listed
    for (unsigned v = 0; v <= 9; ++v) {
        int calls = 0;
        const Err e = dispatch_kinds(v, Invalid, [&](auto K) {
            static_assert(std::is_same_v<typename decltype(K)::value_type, unsigned>);
            constexpr unsigned k = K();  // usable as a template argument
            ++calls;
            CHECK(k == v);
            return Ok;
        });
        const bool listed = v >= 1 && v <= 7;
        CHECK(calls == (listed ? 1 : 0));
        CHECK(e == (listed ? Ok : Invalid));
    }
    // an explicit list with gaps, out of order; a bool fallback (the diag_*_kinds form)
    for (int v = -2; v <= 30; ++v) {
        int got = -100, calls = 0;
        const bool done = dispatch_value<15, 1, 9, 3, 8>(v, false, [&](auto M) {
            static_assert(std::is_same_v<typename decltype(M)::value_type, int>);
            got = std::integral_constant<int, M()>::value;
            ++calls;
            return true;
        });
        const bool listed = v == 15 || v == 1 || v == 9 || v == 3 || v == 8;
        CHECK(done == listed && calls == (listed ? 1 : 0) && got == (listed ? v : -100));
    }
    // a single value; the result type is the fallback's (a pointer here)
    {
        static const char hit[] = "hit";
        const char *miss = nullptr;
        CHECK(dispatch_value<4>(4, miss, [&](auto) { return hit; }) == hit);
        CHECK(dispatch_value<4>(5, miss, [&](auto) { return hit; }) == nullptr);
    }
    // four bools, all 16 inputs: each arrives in the position it was written in
    for (int m = 0; m < 16; ++m) {
        const bool a = m & 1, b = m & 2, c = m & 4, d = m & 8;
        int calls = 0;
        const int r = dispatch_bools(a, b, c, d, [&](auto A, auto B, auto C, auto D) {
            static_assert(std::is_same_v<typename decltype(A)::value_type, bool>);
            ++calls;
            return std::integral_constant<int, (A() ? 1 : 0) | (B() ? 2 : 0) | (C() ? 4 : 0) | (D() ? 8 : 0)>::value;
        });
        CHECK(r == m && calls == 1);
    }
    // one bool, a void lambda, and nesting under a value with if constexpr on both constants
    for (int m = 0; m < 2; ++m) {
        int seen = -1;
        dispatch_bools(m != 0, [&](auto A) { seen = A() ? 1 : 0; });
        CHECK(seen == m);
        const int r = dispatch_value<2, 3>(2 + m, -1, [&](auto P) {
            return dispatch_bools(m == 0, [&](auto F) {
                if constexpr (P() == 3 && F()) return -2;  // never taken: m == 0 goes with P == 2
                else return P() * 10 + (F() ? 1 : 0);
            });
        });
        CHECK(r == (m == 0 ? 21 : 30));
    }
    if (fails == 0) std::printf("dispatch ok\n");
    return fails != 0;
}
