// pnx_tile.hpp -- what the one-lane-per-voxel kernels share (loglinear_kernel, peel_kernel, model_predict_kernel): a block is one
// wave and 64 voxels, and its (64, n) tile of a voxel-major array is contiguous in memory, but a lane's own row is n elements
// from its neighbour's.  So the tile passes through LDS, [voxel][n | 1] doubles (the odd row stride spreads the lanes' rows over
// the banks), and moves to and from memory as 16-byte non-temporal lines, lane after lane.  The helpers own no barrier: the
// kernel puts its __syncthreads() between a tile's lines and its rows.
// The HIP-free argument headers include this file for tile_lds_bytes, and with them the stand-alone host programs of
// tests/host_stub/: device code belongs behind the __HIPCC__ guard below.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pnx {
constexpr int kTileRows = 64;  // voxels of a block: one per lane of its single wave

// LDS of n_tiles such tiles; free of HIP types, the argument headers size their kernels' launches with it
inline size_t tile_lds_bytes(int n_tiles, int n) { return (size_t)n_tiles * kTileRows * (size_t)(n | 1) * sizeof(double); }

#ifdef __HIPCC__
template <typename T> struct Line16;  // 16 bytes of T
template <> struct Line16<double> {
    typedef __attribute__((ext_vector_type(2))) double type;
    static constexpr int N = 2;
};
template <> struct Line16<float> {
    typedef __attribute__((ext_vector_type(4))) float type;
    static constexpr int N = 4;
};

// element e of the (c, n) tile -> its LDS index; inv = 1.0f / n, S = n | 1
__device__ __forceinline__ int tile_at(int e, int n, float inv, int S) {
    int q = (int)((float)e * inv);
    q -= (q * n > e);
    q += ((q + 1) * n <= e);
    return q * S + (e - q * n);
}

// tile <- the n_el = c * n elements of `array` (n per voxel) from voxel v0 on, widened to fp64.  v0 is a multiple of 64, so the
// tile is as aligned as the array itself and the test reads the array's address.  Whole 16-byte lines where it is aligned, the
// last elements one by one; element by element where it is not.
template <typename T> __device__ __forceinline__ void load_tile(double *tile, const T *array, long long v0, int n_el, int n, int lane) {
    typedef typename Line16<T>::type line_t;
    constexpr int V = Line16<T>::N;
    const int S = n | 1;
    const T *src = array + (size_t)v0 * n;
    const float inv = 1.0f / (float)n;
    if (((uintptr_t)array & 15) == 0) {
        for (int e = V * lane; e < n_el; e += V * kTileRows) {
            if (e + V <= n_el) {
                const line_t v = __builtin_nontemporal_load(reinterpret_cast<const line_t *>(src + e));
#pragma unroll
                for (int k = 0; k < V; ++k) tile[tile_at(e + k, n, inv, S)] = (double)v[k];
            } else {
                for (int k = e; k < n_el; ++k) tile[tile_at(k, n, inv, S)] = (double)src[k];
            }
        }
    } else {
        for (int e = lane; e < n_el; e += kTileRows) tile[tile_at(e, n, inv, S)] = (double)src[e];
    }
}

// the mirror image: the n_el elements of `array` from voxel v0 on <- tile
__device__ __forceinline__ void store_tile(double *array, long long v0, const double *tile, int n_el, int n, int lane) {
    typedef Line16<double>::type line_t;
    const int S = n | 1;
    double *dst = array + (size_t)v0 * n;
    const float inv = 1.0f / (float)n;
    if (((uintptr_t)array & 15) == 0) {
        for (int e = 2 * lane; e < n_el; e += 2 * kTileRows) {
            if (e + 1 < n_el) {
                line_t o;
                o.x = tile[tile_at(e, n, inv, S)];
                o.y = tile[tile_at(e + 1, n, inv, S)];
                __builtin_nontemporal_store(o, reinterpret_cast<line_t *>(dst + e));
            } else {
                dst[e] = tile[tile_at(e, n, inv, S)];
            }
        }
    } else {
        for (int e = lane; e < n_el; e += kTileRows) dst[e] = tile[tile_at(e, n, inv, S)];
    }
}
#endif  // __HIPCC__
}  // namespace pnx
