// pcm_write.h -- what the writers among the passes over decoded PCM (pcm_decim.h, pcm_resample.h, pcm_mix.h) share on the
// device.  A writer reads int32 PCM through an input descriptor and writes int32 PCM through an output descriptor: Q30
// products accumulated in int64 (mad), one rounding and the clamp to 16, 20 or 24 bits (finish), the clamped values
// counted per channel -- per thread packed 16 bits a channel, per tile a record of REC words (ClipCount), per stream the
// sum of its tiles' records (join_clipped).  (The requantizer's record has the same shape, and k_rq_join keeps the sum
// written out: with join_clipped its code was other code, and its tool's in-place leg did not stay inside the spread
// of the parent's runs.)
// Everything here is forced inline, and the tile kernels are instruction for instruction what they were with each of
// these written out in them (tools/device_asm_diff.py); what did not pass that check is not here, and says so below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_tiles.h"

namespace pcmw {

constexpr uint32_t REC = pcmt::MAX_CHANNELS;    // words of a tile's record: the clamped values per channel
constexpr uint64_t MAX_FRAME0 = 1ull << 62;     // a piece that says it starts behind this is not taken
// (The rest of take()'s head -- the piece's fields, the test of the two descriptors -- stays written out in pcm_decim.h
// and pcm_resample.h: shared through a function, with or without a struct between the two, every k_dc_tiles and
// k_rs_tiles came out as other code, as k_lvl_join did of PCMT_NOT_TAKEN.)

__host__ __device__ __forceinline__ bool depth_ok(uint32_t b) { return b == 16 || b == 20 || b == 24; }

// acc += coef * x.  On the device the instruction is written out, the coefficient in an SGPR: the compiler's own code for
// `acc += (int64_t)coef * x` is about three slow-class instructions where this is one (each writer says at its tap loop
// what the compiler makes of its coefficients).  (vcc: the carry out nobody reads.)
__host__ __device__ __forceinline__ void mad(int64_t &acc, int32_t coef, int32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_mad_i64_i32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "s"(coef) : "vcc");
#else
    acc += (int64_t)coef * (int64_t)x;
#endif
}

// the one rounding and the clamp; *clipped += 1 when the clamp changed the value
__host__ __device__ __forceinline__ int32_t finish(int64_t acc, uint32_t bits, uint32_t *clipped)
{
    const int64_t q = (acc + (1ll << 29)) >> 30;
    const int64_t hi = (1ll << (bits - 1)) - 1, lo = -hi - 1;
    const int64_t r = q < lo ? lo : q > hi ? hi : q;
    *clipped += r != q ? 1u : 0u;
    return (int32_t)r;
}

// e / d for 0 < d <= 8 and e < 2^24, inv = inv_of(d): 2^32 / d rounded up (d == 1 needs none)
__host__ __device__ __forceinline__ uint32_t inv_of(uint32_t d) { return d > 1 ? 0xFFFFFFFFu / d + 1u : 0u; }
__device__ __forceinline__ uint32_t div_small(uint32_t e, uint32_t d, uint32_t inv) { return d == 1 ? e : __umulhi(e, inv); }

// The clamped values a thread counts over a tile: 16 bits per channel in two 64-bit words (a tile has at most 65 535 per
// channel).  store() folds them over the workgroup (every thread calls it) and thread 0 leaves the tile's record.  No
// atomics; every word a join reads was stored by this launch.  (hi is declared in front of lo: the compiler zeroes the
// two in the order of their declaration, and this is the order in which k_dc_tiles and k_mix_tiles come out as they
// were with the two words written out.  k_rs_tiles keeps them written out: one instance of it moved an instruction.)
struct ClipCount {
    uint64_t hi = 0, lo = 0;
    __device__ __forceinline__ void add(uint32_t c, uint32_t clipped)
    {
        const uint64_t a = (uint64_t)clipped << (16u * (c & 3u));
        lo += c < 4 ? a : 0ull;
        hi += c < 4 ? 0ull : a;
    }
    __device__ __forceinline__ void store(uint32_t *rec_of_tile, uint64_t *s_red)
    {
        lo = pcmt::block_fold(lo, s_red, pcmt::FoldSum());
        hi = pcmt::block_fold(hi, s_red, pcmt::FoldSum());
        if (threadIdx.x == 0) {
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) {
                rec_of_tile[c] = (uint32_t)(lo >> (16u * c)) & 0xFFFFu;
                rec_of_tile[4 + c] = (uint32_t)(hi >> (16u * c)) & 0xFFFFu;
            }
        }
    }
};

// what a join ends with: per channel the sum over the stream's `turns` tile records from record `first` on, zeros for
// the channels at and behind `channels`.  Every thread of the workgroup calls it.
__device__ __forceinline__ void join_clipped(const uint32_t *__restrict__ rec, uint32_t first, uint32_t turns,
                                             uint32_t channels, uint64_t *s_red, uint64_t *clipped)
{
    const uint32_t *r0 = rec + (uint64_t)first * REC;
    for (uint32_t c = 0; c < pcmt::MAX_CHANNELS; c++) {
        uint64_t sum = 0;
        if (c < channels)
            for (uint32_t i = threadIdx.x; i < turns; i += pcmt::THREADS)
                sum += r0[(uint64_t)i * REC + c];
        sum = pcmt::block_fold(sum, s_red, pcmt::FoldSum());
        if (threadIdx.x == 0)
            clipped[c] = sum;
    }
}

} // namespace pcmw
