// pcm_decim.h -- decimation of decoded PCM by D = 2 or 4, on the device: int32 PCM in either int32 layout -> int32 PCM
// in either int32 layout at 1 / D of the rate, every output frame an exact integer FIR over 2 H + 1 input frames
// (N = 96 D - 1 committed integer taps in Q30, pcm_decim_taps.h; 64-bit accumulation; one rounding; clamped to `bits`),
// and per channel the count of the values the clamp changed (include/dvda_mlp_hip.h states the contract).  The sixth
// client of pcm_tiles.h, the first pass that reads across tile seams and the first that changes the frame count.
//
//   value  acc = sum h[k] x[D M - H + k] in int64 (|acc| < 5.2e18 < 2^63 for any int32 input: sum |h| < 2.4e9);
//          y = clamp((acc + 2^29) >> 30).  One text for the kernel and the host: `accumulate` walks a window with the
//          taps as compile-time constants -- a zero tap is no instruction -- for R consecutive outputs at once, and
//          `finish` rounds and clamps.  value<D> is the two with R = 1; dvda_pcm_hip_decim_value compiles it.
//   tiles  TILE OUTPUT frames, aligned to the stream's first output frame.  A workgroup takes a tile in chunks of C
//          output frames, C = chunk_out(channels): the largest of 1024 / 512 / 256 whose staged input fits LDS_WORDS.
//   stage  per channel the chunk's D C + 2 H input frames in LDS, zeros where the region does not hold the frame, so
//          the tap loop has no edge test.  Global loads are 16 bytes where the address allows them (the lanes' groups
//          are shifted to the region's own 16-byte grid), dwords elsewhere; only frames inside `frames` are read.
//          Sample i of a channel lies at word i + i / 16: lanes of the tap loop are 16 samples apart, 17 words
//          in LDS, so their reads fall into different banks.
//   taps   a work item is R = 16 / D consecutive output frames of one channel: R int64 accumulators, the window walked
//          once, each LDS read feeding up to R multiply-adds (pcmw::mad).  Items are dealt to the lanes across
//          channels, C / R per channel.
//   out    planar: 16-byte stores where the plane allows them, else the values one by one; frame-major: dwords, a
//          frame apart (the staged input is still being read, and a value stored is some hundred multiply-adds).
//          Nothing outside the stream's output region is written.
//   count  the clamped values per channel, a record of REC words per tile, summed by the join (pcm_write.h).
//
// tests/decimate_model.py restates the arithmetic with Python integers and in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_decim_taps.h"
#include "pcm_tiles.h"
#include "pcm_write.h"

namespace dcm {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;
using pcmw::depth_ok;
using pcmw::finish;
using pcmw::mad;
using pcmw::MAX_FRAME0;
using pcmw::REC;

constexpr uint32_t TILE = DVDA_DCM_TILE_FRAMES;
constexpr uint32_t TILE_BLOCKS = 4096;      // workgroups of k_dc_tiles at most: they stride over the tile list
constexpr uint32_t LDS_WORDS = 15616;       // of staged input (61 KiB: two workgroups per CU)
constexpr uint32_t LANE_SPAN = 16;          // input samples between two lanes' windows: D * R
static_assert(TILE == 1024 && TILE < (1u << 16), "a tile's counts fit 16 bits");

__host__ __device__ constexpr uint32_t taps_of(uint32_t D) { return 96u * D - 1u; }
__host__ __device__ constexpr uint32_t half_of(uint32_t D) { return 48u * D - 1u; }
__host__ __device__ constexpr uint32_t pad(uint32_t i) { return i + i / LANE_SPAN; }
// words a channel's staged chunk of c_out output frames takes
__host__ __device__ constexpr uint32_t chan_words(uint32_t D, uint32_t c_out) { return pad(D * c_out + 2u * half_of(D)) + 1u; }
__host__ __device__ constexpr uint32_t chunk_out(uint32_t D, uint32_t ch)
{
    return ch * chan_words(D, 1024u) <= LDS_WORDS ? 1024u : ch * chan_words(D, 512u) <= LDS_WORDS ? 512u : 256u;
}
static_assert(MAX_CHANNELS * chan_words(2, 256) <= LDS_WORDS && MAX_CHANNELS * chan_words(4, 256) <= LDS_WORDS,
              "the smallest chunk of eight channels fits");

__host__ __device__ __forceinline__ bool ratio_ok(uint32_t D) { return D == 2 || D == 4; }

// output frames of the absolute frames [frame0, frame0 + own): the M with frame0 <= D M < frame0 + own
__host__ __device__ __forceinline__ uint64_t out_frames(uint64_t frame0, uint64_t own, uint32_t D)
{
    if (!ratio_ok(D) || frame0 > MAX_FRAME0 || own > MAX_FRAME0)
        return 0;
    const uint64_t a = frame0 + own;
    return (a / D + (a % D ? 1u : 0u)) - (frame0 / D + (frame0 % D ? 1u : 0u));
}

// ---- the taps, at compile time
// window position J (sample J of a window that starts H in front of output 0's centre) into the R accumulators: output
// r has its tap J - D r there
template <uint32_t D, uint32_t R, uint32_t J>
__host__ __device__ constexpr bool position_used()
{
    for (uint32_t r = 0; r < R; r++)
        if (J >= D * r && J - D * r < taps_of(D) && Taps<D>::h[J - D * r] != 0)
            return true;
    return false;
}

// A block is BLOCK window positions: its values are loaded while the block in front of it is multiplied, and the
// scheduler is held to that order -- left alone it issues every load of the window first and spills them.
constexpr uint32_t BLOCK = 16;
#if defined(__HIP_DEVICE_COMPILE__)
#define DCM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define DCM_SCHED_FENCE() ((void)0)
#endif

template <uint32_t D, uint32_t R>
__host__ __device__ constexpr uint32_t window_end() { return D * (R - 1u) + taps_of(D); }

template <uint32_t D, uint32_t R, uint32_t J0, uint32_t... Is, class Load>
__host__ __device__ __forceinline__ void load_block(int32_t (&x)[BLOCK], const Load &load, std::integer_sequence<uint32_t, Is...>)
{
    auto one = [&](auto i_) {
        constexpr uint32_t i = decltype(i_)::value;
        if constexpr (J0 + i < window_end<D, R>()) {
            if constexpr (position_used<D, R, J0 + i>())
                x[i] = load(J0 + i);
        }
    };
    (one(std::integral_constant<uint32_t, Is>()), ...);
}

// The multiply-adds are pcmw::mad, each tap a compile-time constant.  From `acc += (int64_t)h * x` the compiler factors
// the symmetric taps, h (x1 + x2), and multiplies that 33-bit sum by h in three instructions where two of the written-out
// one do it.  Its price is the compiler's to set: the hazard recognizer puts an s_nop 0 behind nearly every one, and at
// D = 4 the distinct taps do not fit the scalar file and are rematerialised with s_mov inside the loop.
// tests/test_isa_budget_decimate.py holds every build to the counts DESIGN.md section 17 records.

// position J of the window, value x, into the accumulators of the outputs that have a non-zero tap there
template <uint32_t D, uint32_t R, uint32_t J, uint32_t... Rs>
__host__ __device__ __forceinline__ void position(int64_t (&acc)[R], int32_t x, std::integer_sequence<uint32_t, Rs...>)
{
    auto one = [&](auto r_) {
        constexpr uint32_t r = decltype(r_)::value;
        if constexpr (J >= D * r && J - D * r < taps_of(D)) {
            constexpr int32_t h = Taps<D>::h[J - D * r];
            if constexpr (h != 0)
                mad(acc[r], h, x);
        }
    };
    (one(std::integral_constant<uint32_t, Rs>()), ...);
}

template <uint32_t D, uint32_t R, uint32_t J0, uint32_t... Is>
__host__ __device__ __forceinline__ void mac_block(int64_t (&acc)[R], const int32_t (&x)[BLOCK], std::integer_sequence<uint32_t, Is...>)
{
    auto one = [&](auto i_) {
        constexpr uint32_t i = decltype(i_)::value;
        if constexpr (J0 + i < window_end<D, R>()) {
            if constexpr (position_used<D, R, J0 + i>())
                position<D, R, J0 + i>(acc, x[i], std::make_integer_sequence<uint32_t, R>());
        }
    };
    (one(std::integral_constant<uint32_t, Is>()), ...);
}

template <uint32_t D, uint32_t R, uint32_t J0, class Load>
__host__ __device__ __forceinline__ void blocks_from(int64_t (&acc)[R], const Load &load, const int32_t (&x)[BLOCK])
{
    constexpr auto seq = std::make_integer_sequence<uint32_t, BLOCK>();
    if constexpr (J0 + BLOCK < window_end<D, R>()) {
        int32_t next[BLOCK];
        load_block<D, R, J0 + BLOCK>(next, load, seq);
        mac_block<D, R, J0>(acc, x, seq);
        DCM_SCHED_FENCE();
        blocks_from<D, R, J0 + BLOCK>(acc, load, next);
    } else {
        mac_block<D, R, J0>(acc, x, seq);
    }
}

// acc[r] += sum_k h[k] * load(D r + k), r < R: the window's D (R - 1) + N positions, each loaded once
template <uint32_t D, uint32_t R, class Load>
__host__ __device__ __forceinline__ void accumulate(int64_t (&acc)[R], const Load &load)
{
    int32_t first[BLOCK];
    load_block<D, R, 0>(first, load, std::make_integer_sequence<uint32_t, BLOCK>());
    DCM_SCHED_FENCE();
    blocks_from<D, R, 0>(acc, load, first);
}

// THE value: the output frame whose window of 2 H + 1 input values is window[0 .. 2 H]
template <uint32_t D>
__host__ __device__ __forceinline__ int32_t value(const int32_t *window, uint32_t bits, uint32_t *clipped)
{
    int64_t acc[1] = {0};
    accumulate<D, 1>(acc, [&](uint32_t j) { return window[j]; });
    return finish(acc[0], bits, clipped);
}

// ---- what a stream is to the pass
struct Take {
    uint64_t own;       // frames of the region that are the stream's own (0 when the stream is not taken)
    uint64_t out;       // output frames (0 when the stream is not taken)
    int64_t first;      // region index of output 0's centre
    bool taken;
};

// The input descriptor must be one the reports take and hold its context; the output descriptor must say the same
// channels, exactly the output frames, and have room for them.
__host__ __device__ __forceinline__ Take take(const dvda_pcm_crc_desc &in, const dvda_pcm_crc_desc &out,
                                              const dvda_pcm_decim_piece *piece, uint32_t D)
{
    Take t = {0, 0, 0, false};
    const uint64_t frame0 = piece ? piece->frame0 : 0ull, before = piece ? piece->before : 0u, after = piece ? piece->after : 0u;
    if (PCMT_NOT_TAKEN(in) || before + after > in.frames || frame0 > MAX_FRAME0)
        return t;
    const uint64_t own = in.frames - before - after, o = out_frames(frame0, own, D);
    if (out.channels != in.channels || out.frames != o || out.stride < out.frames)
        return t;
    t.own = own;
    t.out = o;
    t.first = (int64_t)before + (int64_t)((D - frame0 % D) % D);
    t.taken = true;
    return t;
}

__host__ __device__ __forceinline__ uint32_t tiles_of(uint64_t out) { return (uint32_t)((out + TILE - 1) / TILE); }

// ---- step 1: tiles per stream
__global__ void k_dc_plan(const dvda_pcm_crc_desc *__restrict__ desc_in, const dvda_pcm_crc_desc *__restrict__ desc_out,
                          const dvda_pcm_decim_piece *__restrict__ piece, uint32_t n, uint32_t D, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = tiles_of(take(desc_in[i], desc_out[i], piece ? piece + i : nullptr, D).out);
}

// ---- step 3: every tile decimated, and its record.  The workgroups stride over the flat tile list (as many of it as
//      the caller's bound holds: rec has max_tiles records).
template <uint32_t D, bool IN_PLANAR, bool OUT_PLANAR>
__global__ __launch_bounds__(THREADS, 2) void k_dc_tiles(const int32_t *__restrict__ pcm,
                                                      const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                      int32_t *__restrict__ out,
                                                      const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                      const dvda_pcm_decim_piece *__restrict__ piece, uint32_t n,
                                                      uint32_t bits, const uint32_t *__restrict__ base,
                                                      uint32_t *__restrict__ rec, uint32_t max_tiles)
{
    constexpr uint32_t R = LANE_SPAN / D, H = half_of(D);
    __shared__ __attribute__((aligned(16))) uint32_t s_buf[LDS_WORDS];
    __shared__ uint64_t s_red[WAVES];
    const uint32_t t = threadIdx.x;
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc di = desc_in[s], dn = desc_out[s];
        const Take tk = take(di, dn, piece ? piece + s : nullptr, D);
        const uint32_t ti = b - base[s];
        if (ti >= tiles_of(tk.out))         // (counts that wrapped the scan: no tile of this stream, nothing is touched)
            continue;
        const uint32_t ch = di.channels;
        const uint64_t m0 = (uint64_t)ti * TILE;                                    // the tile's first output frame
        const uint32_t nm = tk.out - m0 < TILE ? (uint32_t)(tk.out - m0) : TILE;    // ... and how many it has
        const uint32_t C = chunk_out(D, ch), CS = chan_words(D, C), L = D * C + 2u * H;
        const uint32_t per_ch = C / R;      // work items of a channel (a power of two)
        const int32_t *in_s = pcm + di.off;
        int32_t *out_s = out + dn.off;
        const bool out_16 = (reinterpret_cast<uintptr_t>(out_s) & 15u) == 0 && (ch == 1 || (dn.stride & 3u) == 0);
        pcmw::ClipCount cnt;
        for (uint32_t k0 = 0; k0 < nm; k0 += C) {
            const uint32_t nmc = nm - k0 < C ? nm - k0 : C;                         // output frames of the chunk
            // region index of staged sample 0: H in front of the centre of the chunk's first output
            const int64_t j0 = tk.first + (int64_t)D * (int64_t)(m0 + k0) - (int64_t)H;
            // ---- stage: sample i of channel c -> s_buf[c * CS + pad(i)], zero where the region does not hold it
            if (IN_PLANAR) {
                for (uint32_t c = 0; c < ch; c++) {
                    const int32_t *plane = in_s + (uint64_t)c * di.stride;
                    // the groups of four lie on memory's 16-byte grid: the first starts `sh` samples in front of sample 0
                    const uint32_t sh = (uint32_t)((int64_t)(reinterpret_cast<uintptr_t>(plane) >> 2) + j0) & 3u;
                    uint32_t *sc = s_buf + c * CS;
                    for (uint32_t q = t; 4u * q < L + sh; q += THREADS) {
                        const int64_t j = j0 + (int64_t)(4u * q) - (int64_t)sh;    // region index of the group's first
                        int32_t v[4] = {0, 0, 0, 0};
                        if (j >= 0 && j + 4 <= (int64_t)di.frames) {
                            const int4 g = *reinterpret_cast<const int4 *>(plane + j);
                            v[0] = g.x, v[1] = g.y, v[2] = g.z, v[3] = g.w;
                        } else {
#pragma unroll
                            for (uint32_t e = 0; e < 4; e++)
                                if (j + e >= 0 && j + e < (int64_t)di.frames)
                                    v[e] = plane[j + e];
                        }
#pragma unroll
                        for (uint32_t e = 0; e < 4; e++) {
                            const uint32_t i = 4u * q + e - sh;         // (wraps below 0: not < L)
                            if (i < L)
                                sc[pad(i)] = (uint32_t)v[e];
                        }
                    }
                }
            } else {
                // the chunk's frames are one run of L * ch dwords; dword w of it is sample w / ch of channel w % ch
                const int64_t w0 = j0 * (int64_t)ch, w_end = (int64_t)di.frames * ch;
                const uint32_t sh = (uint32_t)((int64_t)(reinterpret_cast<uintptr_t>(in_s) >> 2) + w0) & 3u;
                const uint32_t nw = L * ch;
                for (uint32_t q = t; 4u * q < nw + sh; q += THREADS) {
                    const int64_t w = w0 + (int64_t)(4u * q) - (int64_t)sh;
                    int32_t v[4] = {0, 0, 0, 0};
                    if (w >= 0 && w + 4 <= w_end) {
                        const int4 g = *reinterpret_cast<const int4 *>(in_s + w);
                        v[0] = g.x, v[1] = g.y, v[2] = g.z, v[3] = g.w;
                    } else {
#pragma unroll
                        for (uint32_t e = 0; e < 4; e++)
                            if (w + e >= 0 && w + e < w_end)
                                v[e] = in_s[w + e];
                    }
                    const uint32_t first = 4u * q >= sh ? 4u * q - sh : 0u;        // the group's first dword inside the run
                    uint32_t i = first / ch, c = first - i * ch;
#pragma unroll
                    for (uint32_t e = 0; e < 4; e++) {
                        const uint32_t d = 4u * q + e - sh;             // (wraps below 0: not < nw)
                        if (d < nw) {
                            s_buf[c * CS + pad(i)] = (uint32_t)v[e];
                            if (++c == ch)
                                c = 0, i++;
                        }
                    }
                }
            }
            __syncthreads();
            // ---- taps: item `it` is the outputs R g .. R g + R - 1 of the chunk in channel c
            const uint32_t items = ch * per_ch;
            for (uint32_t it = t; it < items; it += THREADS) {
                const uint32_t c = it / per_ch, g = it % per_ch;
                const uint32_t o0 = R * g;                              // the item's first output frame in the chunk
                if (o0 >= nmc)
                    continue;
                const int32_t *win = reinterpret_cast<const int32_t *>(s_buf) + c * CS + (LANE_SPAN + 1u) * g;
                int64_t acc[R];
#pragma unroll
                for (uint32_t r = 0; r < R; r++)
                    acc[r] = 0;
                accumulate<D, R>(acc, [&](uint32_t j) { return win[pad(j)]; });
                int32_t y[R];
                uint32_t cl = 0;
#pragma unroll
                for (uint32_t r = 0; r < R; r++) {
                    uint32_t one = 0;
                    y[r] = finish(acc[r], bits, &one);
                    cl += o0 + r < nmc ? one : 0u;                      // (behind the stream's end: not an output)
                }
                cnt.add(c, cl);
                const uint64_t m = m0 + k0 + o0;                        // the item's first output frame in the stream
                if (OUT_PLANAR) {
                    int32_t *o = out_s + (uint64_t)c * dn.stride + m;
                    if (out_16 && o0 + R <= nmc) {
#pragma unroll
                        for (uint32_t r = 0; r < R; r += 4)
                            *reinterpret_cast<int4 *>(o + r) = make_int4(y[r], y[r + 1], y[r + 2], y[r + 3]);
                    } else {
#pragma unroll
                        for (uint32_t r = 0; r < R; r++)
                            if (o0 + r < nmc)
                                o[r] = y[r];
                    }
                } else {
                    // (dwords, a frame apart: the staged input is still being read by other items, and the pass is
                    //  bound by its multiply-adds, some hundred per value stored)
                    int32_t *o = out_s + m * ch + c;
#pragma unroll
                    for (uint32_t r = 0; r < R; r++)
                        if (o0 + r < nmc)
                            o[(uint64_t)r * ch] = y[r];
                }
            }
            __syncthreads();            // (s_buf has been read: the next chunk fills it)
        }
        cnt.store(rec + (uint64_t)b * REC, s_red);
    }
}

// ---- step 4: one workgroup per stream sums the stream's records.  A stream whose tiles do not all lie inside the
//      caller's bound is reported as zeros, as one that is not taken.
__global__ __launch_bounds__(THREADS) void k_dc_join(const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                     const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                     const dvda_pcm_decim_piece *__restrict__ piece, uint32_t n, uint32_t D,
                                                     const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                     uint32_t max_tiles, dvda_pcm_decim_report *__restrict__ out)
{
    __shared__ uint64_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    const Take tk = take(desc_in[s], desc_out[s], piece ? piece + s : nullptr, D);
    const uint32_t first = base[s], n_t = tiles_of(tk.out);
    const bool taken = tk.taken && (uint64_t)first + n_t <= max_tiles;
    if (threadIdx.x == 0) {
        out[s].frames_in = taken ? tk.own : 0ull;
        out[s].frames_out = taken ? tk.out : 0ull;
    }
    pcmw::join_clipped(rec, first, taken ? n_t : 0u, taken ? desc_in[s].channels : 0u, s_red, out[s].clipped);
}

} // namespace dcm
