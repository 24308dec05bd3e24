// The layout of one partial Gram of zgram.hip and the fixed tree that sums partials, shared by
// the kernels that read partials (zgram.hip's trees, xsreg.hip's solve from parts).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace afm {

// tile shape of a p-regressor design: 2 tiles (p + 2 <= 32) or 7 (p + 2 <= 108)
constexpr int zgram_nt(int p) { return p + 2 <= 32 ? 2 : 7; }
// doubles of one partial: the NT (NT + 1) / 2 upper-triangle 16 x 16 tile pairs, 256 each
constexpr int zgram_pe(int nt) { return nt * (nt + 1) / 2 * 256; }

// Element e of a partial -> (row, col) of the Gram: tile pair q = e / 256 of the J-major
// upper-triangle list (ZPairs in zgram.hip), then the f64 MFMA C/D layout inside the tile.
__device__ __forceinline__ void zgram_elem_rc(int e, int& row, int& col) {
    int i = e >> 8, j = 0;
    while (i > j) { i -= j + 1; ++j; }
    const int r = (e >> 6) & 3, lane = e & 63;
    row = i * 16 + (lane >> 4) + 4 * r;
    col = j * 16 + (lane & 15);
}

// The fixed tree over the leaves v[0..n) (n <= 32; v[b] for b >= n is never read): strides 1, 2,
// 4, 8, 16, v[i] += v[i+s] for i a multiple of 2s.  Every kernel that merges partials sums
// through this one function, so a fused launch adds what the separate launches added, in the
// same order.
__device__ __forceinline__ double zgram_tree32(double (&v)[32], int n) {
#pragma unroll
    for (int s = 1; s < 32; s *= 2)
#pragma unroll
        for (int i = 0; i + s < 32; i += 2 * s)
            if (i + s < n) v[i] = v[i] + v[i + s];
    return v[0];
}

}  // namespace afm
