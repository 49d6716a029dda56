// The scan layer shared by the sort (fgs_sort.hip), the binning (fgs_bin.hip) and the surface generator (fgs_surface.hip):
// the wave-wide inclusive scan and the exclusive scan over a 256-thread block built on it.  wave64 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Inclusive sum over the wave's lanes 0 ... own.
static __device__ __forceinline__ uint32_t wave_incl_scan(uint32_t s) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(s, o, 64);
        if ((int)lane >= o) s += t;
    }
    return s;
}

// exclusive scan of one value per thread over a 256-thread block; returns block total in *tot
static __device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t *tot) {
    __shared__ uint32_t wsum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t s = wave_incl_scan(v);
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t x = wsum[w];
        pre += (w < (int)wave) ? x : 0u;
        all += x;
    }
    *tot = all;
    return pre + s - v;
}
