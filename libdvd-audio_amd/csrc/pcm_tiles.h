// pcm_tiles.h -- what the reports of decoded PCM (pcm_digest.h, pcm_levels.h, pcm_compare.h, pcm_energy.h, pcm_requant.h, pcm_decim.h, pcm_resample.h, pcm_mix.h) share on the device: a descriptor per
// stream, a flat list of tiles over all streams (tiles per stream -> exclusive scan `base` -> one workgroup per tile ->
// one workgroup per stream joins its tiles), workgroups of WAVES waves.  The host side of the list: pcm_report_run.h.
// What only the writers share (decimate, resample, mix): pcm_write.h -- the written-out multiply-add,
// the rounding and the clamp, the depth test, the small division, the packed count of clamped values and the joins' sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"

namespace pcmt {

constexpr int WAVES = 4;
constexpr int THREADS = WAVES * 64;
constexpr uint32_t MAX_CHANNELS = 8;

// A descriptor outside what the kernels take -- no channels or more than these, more frames -- is an empty stream.
// (Shared as text, not as a function: called through one, the compiler makes other code of k_lvl_join than of the
// condition written out where it is used, and both reports' measurements were taken on the code as it is.)
#define PCMT_NOT_TAKEN(d) ((d).channels == 0 || (d).channels > pcmt::MAX_CHANNELS || (d).frames > (1ull << 40))

// the stream that holds tile `b` of the flat list: the last one whose base is at or before b (streams without tiles
// share their base with the stream behind them and are passed over)
__host__ __device__ __forceinline__ uint32_t find_stream(const uint32_t *__restrict__ base, uint32_t n, uint32_t b)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// tiles of the flat list a tile kernel walks: all of them, or as many as the caller's bound holds
__device__ __forceinline__ uint32_t list_tiles(const uint32_t *__restrict__ base, uint32_t n, uint32_t max_tiles)
{
    const uint32_t total = base[n];
    return total > max_tiles ? max_tiles : total;
}

// A fold over the workgroup: over the wave by shuffles, over the waves through s_red (WAVES words).  Every thread calls
// it, thread 0 holds the result.  Op: T operator()(T, T), and T start(T own): what thread 0 folds the waves' values
// into -- the neutral value, or its own wave's value where that is neutral (a minimum).
template <typename T, typename Op>
__device__ __forceinline__ T block_fold(T v, T *s_red, Op op)
{
    for (int o = 32; o; o >>= 1)
        v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();                    // (s_red of the turn before has been read)
    if ((threadIdx.x & 63u) == 0)
        s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = op.start(v);
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; w++)
            r = op(r, s_red[w]);
    return r;
}

struct FoldXor {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a ^ b; }
    __device__ __forceinline__ uint32_t start(uint32_t) const { return 0u; }
};
struct FoldMin {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return b < a ? b : a; }
    __device__ __forceinline__ uint64_t start(uint64_t own) const { return own; }
};
struct FoldSum {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
    __device__ __forceinline__ uint64_t start(uint64_t) const { return 0ull; }
};

} // namespace pcmt
