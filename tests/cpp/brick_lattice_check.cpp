// csrc/brick_lattice.hpp on its own (no HIP): brick_holders against a brute-force list of the (brick, patch
// position) pairs that hold a lattice dof, as a sequence (the order fixes the bits of every sum over a dof's
// patch entries), on full and cut lattices; and xcd_order as a permutation with a contiguous range per XCD.
#include <array>
#include <cstdio>
#include <vector>

#include "brick_lattice.hpp"

using namespace cdfem;

static int fails = 0;
static long long checked = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++fails <= 20) { std::printf("FAIL line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                     \
    } while (0)

using Hold = std::array<int, 6>;  // bx, by, bz, px, py, pz

// every dof of an Lx x Ly x Lz lattice over nb bricks of S x S x SZ patches (origins (S - 1) b, (SZ - 1) bz)
template <int S, int SZ>
static void check_lattice(const int (&nb)[3], int Lx, int Ly, int Lz)
{
    for (int gz = 0; gz < Lz; ++gz)
        for (int gy = 0; gy < Ly; ++gy)
            for (int gx = 0; gx < Lx; ++gx) {
                std::vector<Hold> want, got;
                // brute force: all bricks, z outermost and the lower brick first on every axis
                for (int bz = 0; bz < nb[2]; ++bz)
                    for (int by = 0; by < nb[1]; ++by)
                        for (int bx = 0; bx < nb[0]; ++bx) {
                            const int px = gx - (S - 1) * bx, py = gy - (S - 1) * by, pz = gz - (SZ - 1) * bz;
                            if (px >= 0 && px < S && py >= 0 && py < S && pz >= 0 && pz < SZ)
                                want.push_back(Hold{bx, by, bz, px, py, pz});
                        }
                brick_holders<S, SZ>(nb[0], nb[1], nb[2], gx, gy, gz, [&](int bx, int by, int bz, int px, int py, int pz) {
                    got.push_back(Hold{bx, by, bz, px, py, pz});
                });
                const size_t n = got.size();
                CHECK(n == 1 || n == 2 || n == 4 || n == 8, "S %d SZ %d dof (%d, %d, %d): %zu holders", S, SZ, gx, gy, gz, n);
                CHECK(got == want, "S %d SZ %d nb (%d, %d, %d) L (%d, %d, %d) dof (%d, %d, %d): %zu holders, %zu by brute force",
                      S, SZ, nb[0], nb[1], nb[2], Lx, Ly, Lz, gx, gy, gz, n, want.size());
                ++checked;
            }
}

template <int S, int SZ>
static void check_patch()
{
    const int grids[3][3] = {{1, 1, 1}, {2, 1, 3}, {3, 2, 2}};
    for (const auto &nb : grids) {
        // the full lattice, and the last brick cut to c planes (2 <= c < S: the previous brick's face and c - 1
        // planes past it) on one, two and three axes; the last case leaves a single plane past the face on z
        const int fx = nb[0] * (S - 1) + 1, fy = nb[1] * (S - 1) + 1, fz = nb[2] * (SZ - 1) + 1;
        auto cut = [](int full, int s1, int c) { return full - s1 - 1 + c; };
        check_lattice<S, SZ>(nb, fx, fy, fz);
        check_lattice<S, SZ>(nb, cut(fx, S - 1, 3), fy, fz);
        check_lattice<S, SZ>(nb, fx, cut(fy, S - 1, S - 1), cut(fz, SZ - 1, SZ / 2));
        check_lattice<S, SZ>(nb, cut(fx, S - 1, S - 2), cut(fy, S - 1, 2), cut(fz, SZ - 1, SZ - 1));
        check_lattice<S, SZ>(nb, fx, cut(fy, S - 1, 4), cut(fz, SZ - 1, 2));
    }
}

static void check_xcd_order()
{
    for (unsigned G = 1; G <= 70; ++G) {
        std::vector<int> seen(G, 0);
        int lo[8] = {}, hi[8] = {}, cnt[8] = {};
        for (unsigned b = 0; b < G; ++b) {
            const int v = xcd_order(b, G);
            CHECK(v >= 0 && v < (int)G, "G %u b %u -> %d", G, b, v);
            if (v < 0 || v >= (int)G) continue;
            ++seen[v];
            const unsigned x = b % 8;
            lo[x] = cnt[x] ? (v < lo[x] ? v : lo[x]) : v;
            hi[x] = cnt[x] ? (v > hi[x] ? v : hi[x]) : v;
            ++cnt[x];
        }
        for (unsigned v = 0; v < G; ++v) CHECK(seen[v] == 1, "G %u: brick %u taken %d times", G, v, seen[v]);
        if (G % 8 == 0)
            for (int x = 0; x < 8; ++x)
                CHECK(cnt[x] == (int)G / 8 && hi[x] - lo[x] + 1 == cnt[x], "G %u XCD %d: %d bricks in [%d, %d]", G, x, cnt[x], lo[x], hi[x]);
    }
}

int main()
{
    check_patch<5, 5>();
    check_patch<9, 9>();
    check_patch<7, 7>();
    check_patch<7, 13>();
    check_patch<9, 17>();
    check_xcd_order();
    CHECK(checked > 100000, "only %lld dofs were checked", checked);
    if (fails) {
        std::printf("%d failures\n", fails);
        return 1;
    }
    std::printf("brick lattice ok (%lld dofs)\n", checked);
    return 0;
}
