// brick_lattice.hpp — the index rules of the brick lattice that need no HIP: the XCD brick order and the 1-8
// (brick, patch position) pairs that hold a lattice dof.  Plain C++ (tests/cpp/brick_lattice_check.cpp builds
// it with g++); included by brick_core.hpp.
#pragma once

#ifdef __HIPCC__
#define CDFEM_LATTICE_FN __host__ __device__ __forceinline__
#else
#define CDFEM_LATTICE_FN inline
#endif

namespace cdfem {

// Workgroup b of a grid of G runs on XCD b % 8; this order gives each XCD a contiguous range of bricks, so
// a brick's neighbours (which re-read its patch faces) are mostly on the same L2.  A permutation of 0 .. G - 1.
CDFEM_LATTICE_FN int xcd_order(unsigned b, unsigned G)
{
    const unsigned x = b % 8, k = b / 8, q = G / 8, r = G % 8;
    return (int)(x * q + (x < r ? x : r) + k);
}

// f(bx, by, bz, px, py, pz) for every brick of an nbx x nby x nbz grid whose S x S x SZ patch holds lattice dof
// (gx, gy, gz), with the dof's position in that patch: 1 pair inside a patch, 2 / 4 / 8 on a brick face / edge /
// corner.  The order is the one every sum over a dof's patch entries takes (patch_sum8, the update, the face
// sums, the slab's plane sums): lower brick first per axis, z outermost.
template <int S, int SZ = S, typename F>
CDFEM_LATTICE_FN void brick_holders(int nbx, int nby, int nbz, int gx, int gy, int gz, F &&f)
{
    // per axis: the holders of coordinate g = q s1 + p are brick q at p, and where p = 0 also brick q - 1 at s1
    // (none below the first brick, and the last lattice plane of a full axis has q = nb: brick q - 1 alone).
    // Selects, no indexed arrays: the device keeps everything in registers.
    struct Axis {
        int n, b0, p0;  // n holders; the first is brick b0 at p0, a second is brick b0 + 1 at 0
    };
    auto axis = [](int g, int s1, int nb) {
        const int q = g / s1, p = g - q * s1;
        const bool lower = p == 0 && q - 1 >= 0;
        return Axis{lower ? (q < nb ? 2 : 1) : 1, lower ? q - 1 : q, lower ? s1 : p};
    };
    const Axis X = axis(gx, S - 1, nbx), Y = axis(gy, S - 1, nby), Z = axis(gz, SZ - 1, nbz);
    for (int kz = 0; kz < Z.n; ++kz)
        for (int ky = 0; ky < Y.n; ++ky)
            for (int kx = 0; kx < X.n; ++kx)
                f(X.b0 + kx, Y.b0 + ky, Z.b0 + kz, kx ? 0 : X.p0, ky ? 0 : Y.p0, kz ? 0 : Z.p0);
}

}  // namespace cdfem

#undef CDFEM_LATTICE_FN
