// pcm_resample.h -- 48 kHz to 44.1 kHz on the device: int32 PCM in either int32 layout -> int32 PCM in either int32
// layout at 147 / 160 of the rate, every output frame an exact integer FIR over 96 input frames whose taps are one of
// 147 phases (the committed table g[147][96] in Q30, pcm_resample_taps.h; 64-bit accumulation; one rounding; clamped to
// `bits`), and per channel the count of the values the clamp changed (include/dvda_mlp_hip.h states the contract).  The
// seventh client of pcm_tiles.h and the first pass whose taps differ from output frame to output frame.
//
//   value  output m (absolute): q = (160 m) div 147, p = (160 m) mod 147, acc = sum_i g[p][i] x[q - 47 + i] in int64
//          (sum |g| < 2^32: no int32 input overflows it), y = clamp((acc + 2^29) >> 30).  One text for the kernel and the
//          host: `accumulate` walks a window for R consecutive outputs at once, `finish` rounds and clamps; value() is
//          the two with R = 1 and dvda_pcm_hip_resample_value compiles it.
//   phase  outputs 147 apart share their phase and their inputs are 160 apart: output 147 K + r of a stream is "block K,
//          residue r".  A wave takes one group of R = 3 consecutive residues at a time and its 64 lanes are 64 (block,
//          channel) pairs, so the 3 tap rows are the same in every lane: wave-uniform pointers into the table, read with
//          scalar loads, the multiply-add's tap operand an SGPR.
//   window consecutive outputs step the input by 1 or 2 frames, depending on the phase.  The table the kernel reads is
//          the committed one with R - 1 zeros on either side of every row (Padded): output k of a group multiplies the
//          window positions k .. k + 95 + k, its row's pointer shifted by how far its window really starts behind
//          output 0's, so the lane's window of 96 + 2 (R - 1) values is indexed statically and each LDS read feeds up to
//          R multiply-adds -- 291 of them per group, 3 more than the 288 of the arithmetic.
//   tiles  TILE = 64 blocks = 9 408 OUTPUT frames, aligned to the stream's first output frame.  A workgroup takes a tile
//          in chunks of 64 / channels blocks: 64 pairs at most.
//   stage  per pair the block's 255 input frames (160 window starts + 95) in LDS at pair * 255, zeros where the region
//          does not hold the frame, so the tap loop has no edge test; blocks overlap by 95 frames and those are staged
//          twice.  255 is odd: the lanes of the tap loop, one pair apart, read 64 different banks.  Only frames inside
//          `frames` are read (dwords: the pass is bound by its multiply-adds, 96 per value, not by its loads).
//   out    dwords, straight from the registers; nothing outside the stream's output region is written.
//   count  the clamped values per channel, a record of REC words per tile, summed by the join: pcm_write.h's record,
//          packed and stored here as pcmw::ClipCount does it (written out: see there).
//
// tests/resample_model.py restates the arithmetic with Python integers and in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_resample_taps.h"
#include "pcm_tiles.h"
#include "pcm_write.h"

namespace rsm {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;
using pcmw::depth_ok;
using pcmw::div_small;
using pcmw::finish;
using pcmw::mad;
using pcmw::MAX_FRAME0;
using pcmw::REC;

constexpr uint32_t UP = PHASES, DOWN = 160; // out = in * UP / DOWN
constexpr uint32_t FRONT = 47;              // input frames of a window in front of frame q
constexpr uint32_t TILE = DVDA_RSM_TILE_FRAMES;
constexpr uint32_t TILE_BLOCKS = 4096;      // workgroups of k_rs_tiles at most: they stride over the tile list
constexpr uint32_t PAIRS = 64;              // (block, channel) pairs of a chunk: the lanes of a wave
constexpr uint32_t R = 3;                   // consecutive outputs of a work item
constexpr uint32_t GROUPS = UP / R;         // work items of a pair
constexpr uint32_t SPAN = DOWN + TAPS - 1;  // input frames a block's windows cover
constexpr uint32_t WINDOW = TAPS + 2 * (R - 1);     // window positions of a work item
constexpr uint32_t LDS_WORDS = PAIRS * SPAN + 2;    // (the last pair's last item reads two words behind its span, times 0)
static_assert(TILE == PAIRS * UP && TILE < (1u << 16), "a tile is 64 blocks and its counts fit 16 bits");
// (an item's last output starts at most DOWN - 1 into the span, and at least R - 1 behind its first)
static_assert(GROUPS * R == UP && (SPAN & 1u) == 1 && DOWN - R + WINDOW <= SPAN + 2, "groups tile a block; odd LDS stride");

// ceil(147 a / 160) without the product
__host__ __device__ __forceinline__ uint64_t first_out(uint64_t a)
{
    return (uint64_t)UP * (a / DOWN) + ((uint64_t)UP * (a % DOWN) + DOWN - 1) / DOWN;
}

// output frames of the absolute frames [frame0, frame0 + own): the m with frame0 <= (160 m) div 147 < frame0 + own
__host__ __device__ __forceinline__ uint64_t out_frames(uint64_t frame0, uint64_t own)
{
    if (frame0 > MAX_FRAME0 || own > MAX_FRAME0)
        return 0;
    return first_out(frame0 + own) - first_out(frame0);
}

// ---- the table the tap loop reads: every row with R - 1 zeros in front of it and behind it
struct Padded {
    int32_t v[PHASES][TAPS + 2 * (R - 1)];
};
constexpr Padded padded()
{
    Padded t = {};
    for (uint32_t p = 0; p < PHASES; p++)
        for (uint32_t i = 0; i < TAPS; i++)
            t.v[p][R - 1 + i] = Table::g[p][i];
    return t;
}
#if defined(__HIP_DEVICE_COMPILE__)
__constant__ const Padded PAD = padded();
#else
static const Padded PAD = padded();
#endif

// residue s (an output frame mod 147): how far its window starts behind that of residue 0, and its phase
__host__ __device__ __forceinline__ uint32_t start_of(uint32_t s) { return DOWN * s / UP; }
__host__ __device__ __forceinline__ uint32_t phase_of(uint32_t s) { return DOWN * s % UP; }

// the row of output k of a work item: its window starts `shift` positions behind position k, 0 <= shift <= k
__host__ __device__ __forceinline__ const int32_t *row_of(uint32_t phase, uint32_t shift) { return PAD.v[phase] + (R - 1 - shift); }

// The multiply-adds are pcmw::mad, the tap wave-uniform in an SGPR: from `acc += (int64_t)g * x` with such a g the
// compiler extends the tap to 64 bits on the scalar side and multiplies in pieces (v_mad_u64_u32, v_mul_lo_u32, adds).

// A block is BLOCK window positions: its values (LDS) and its taps (scalar loads) are asked for while the block in front
// of it is multiplied.  The scheduler is held to that order, and the wave waits for the block it is about to multiply
// BEFORE it asks for the next one: scalar loads return out of order, so the only wait there is for them is "everything
// asked for so far", and placed by the compiler at the first multiply it would wait for the block just asked for too.
constexpr uint32_t BLOCK = 8;
#if defined(__HIP_DEVICE_COMPILE__)
#define RSM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define RSM_WAIT_LOADS() __builtin_amdgcn_s_waitcnt(0xC07F)        /* lgkmcnt(0), the other counters left alone */
#else
#define RSM_SCHED_FENCE() ((void)0)
#define RSM_WAIT_LOADS() ((void)0)
#endif

template <uint32_t N>
__host__ __device__ constexpr uint32_t positions() { return TAPS + 2u * (N - 1u); }
// position j of the window is tap j - k of output k's padded row
template <uint32_t N>
__host__ __device__ constexpr bool reaches(uint32_t j, uint32_t k) { return j >= k && j - k < TAPS + k; }

template <uint32_t N>
struct Block {
    int32_t x[BLOCK];
    int32_t g[N][BLOCK];
};

template <uint32_t N, uint32_t J0, class Load>
__host__ __device__ __forceinline__ void load_block(Block<N> &b, const int32_t *const (&row)[N], const Load &load)
{
#pragma unroll
    for (uint32_t i = 0; i < BLOCK; i++) {
        const uint32_t j = J0 + i;
        if (j < positions<N>()) {
            b.x[i] = load(j);
#pragma unroll
            for (uint32_t k = 0; k < N; k++)
                if (reaches<N>(j, k))
                    b.g[k][i] = row[k][j - k];
        }
    }
}

template <uint32_t N, uint32_t J0>
__host__ __device__ __forceinline__ void mac_block(int64_t (&acc)[N], const Block<N> &b)
{
#pragma unroll
    for (uint32_t i = 0; i < BLOCK; i++) {
        const uint32_t j = J0 + i;
        if (j < positions<N>()) {
#pragma unroll
            for (uint32_t k = 0; k < N; k++)
                if (reaches<N>(j, k))
                    mad(acc[k], b.g[k][i], b.x[i]);
        }
    }
}

template <uint32_t N, uint32_t J0, class Load>
__host__ __device__ __forceinline__ void blocks_from(int64_t (&acc)[N], const int32_t *const (&row)[N], const Load &load,
                                                     const Block<N> &cur)
{
    if constexpr (J0 + BLOCK < positions<N>()) {
        Block<N> next;
        RSM_WAIT_LOADS();
        RSM_SCHED_FENCE();
        load_block<N, J0 + BLOCK>(next, row, load);
        RSM_SCHED_FENCE();
        mac_block<N, J0>(acc, cur);
        RSM_SCHED_FENCE();
        blocks_from<N, J0 + BLOCK>(acc, row, load, next);
    } else {
        mac_block<N, J0>(acc, cur);
    }
}

// acc[k] += sum_i g[p_k][i] * load(start_k + i), k < N, where row[k] = row_of(p_k, start_k - k): the window's positions
// walked once, position j into every output whose (padded) row reaches it
template <uint32_t N, class Load>
__host__ __device__ __forceinline__ void accumulate(int64_t (&acc)[N], const int32_t *const (&row)[N], const Load &load)
{
    Block<N> first;
    load_block<N, 0>(first, row, load);
    RSM_SCHED_FENCE();
    blocks_from<N, 0>(acc, row, load, first);
}

// THE value: the output frame of phase `phase` whose window of 96 input values is window[0 .. 95]
__host__ __device__ __forceinline__ int32_t value(const int32_t *window, uint32_t phase, uint32_t bits, uint32_t *clipped)
{
    int64_t acc[1] = {0};
    const int32_t *const row[1] = {PAD.v[phase] + (R - 1)};
    accumulate<1>(acc, row, [&](uint32_t j) { return window[j]; });
    return finish(acc[0], bits, clipped);
}

// ---- what a stream is to the pass
struct Take {
    uint64_t own;       // frames of the region that are the stream's own (0 when the stream is not taken)
    uint64_t out;       // output frames (0 when the stream is not taken)
    int64_t rel;        // region index of the first staged frame of block 0: blocks are 160 frames apart
    uint32_t b;         // the stream's first output frame mod 147
    bool taken;
};

// The input descriptor must be one the reports take and hold its context; the output descriptor must say the same
// channels, exactly the output frames, and have room for them.
__host__ __device__ __forceinline__ Take take(const dvda_pcm_crc_desc &in, const dvda_pcm_crc_desc &out,
                                              const dvda_pcm_decim_piece *piece)
{
    Take t = {0, 0, 0, 0, false};
    const uint64_t frame0 = piece ? piece->frame0 : 0ull, before = piece ? piece->before : 0u, after = piece ? piece->after : 0u;
    if (PCMT_NOT_TAKEN(in) || before + after > in.frames || frame0 > MAX_FRAME0)
        return t;
    const uint64_t own = in.frames - before - after, o = out_frames(frame0, own);
    if (out.channels != in.channels || out.frames != o || out.stride < out.frames)
        return t;
    const uint64_t m = first_out(frame0);           // the stream's first output frame: block m / 147, residue m % 147
    t.own = own;
    t.out = o;
    t.b = (uint32_t)(m % UP);
    // the absolute frame block 0's staged span starts at, then the region's index of it
    t.rel = (int64_t)((uint64_t)DOWN * (m / UP)) + (int64_t)start_of(t.b) - (int64_t)FRONT - (int64_t)frame0 + (int64_t)before;
    t.taken = true;
    return t;
}

__host__ __device__ __forceinline__ uint32_t tiles_of(uint64_t out) { return (uint32_t)((out + TILE - 1) / TILE); }

// ---- step 1: tiles per stream
__global__ void k_rs_plan(const dvda_pcm_crc_desc *__restrict__ desc_in, const dvda_pcm_crc_desc *__restrict__ desc_out,
                          const dvda_pcm_decim_piece *__restrict__ piece, uint32_t n, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = tiles_of(take(desc_in[i], desc_out[i], piece ? piece + i : nullptr).out);
}

// ---- step 3: every tile resampled, and its record.  The workgroups stride over the flat tile list (as many of it as
//      the caller's bound holds: rec has max_tiles records).
template <bool IN_PLANAR, bool OUT_PLANAR>
__global__ __launch_bounds__(THREADS, 2) void k_rs_tiles(const int32_t *__restrict__ pcm,
                                                      const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                      int32_t *__restrict__ out,
                                                      const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                      const dvda_pcm_decim_piece *__restrict__ piece, uint32_t n,
                                                      uint32_t bits, const uint32_t *__restrict__ base,
                                                      uint32_t *__restrict__ rec, uint32_t max_tiles)
{
    __shared__ uint32_t s_buf[LDS_WORDS];
    __shared__ uint64_t s_red[WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc di = desc_in[s], dn = desc_out[s];
        const Take tk = take(di, dn, piece ? piece + s : nullptr);
        const uint32_t ti = b - base[s];
        if (ti >= tiles_of(tk.out))         // (counts that wrapped the scan: no tile of this stream, nothing is touched)
            continue;
        const uint32_t ch = di.channels, inv = pcmw::inv_of(ch);
        const uint64_t m0 = (uint64_t)ti * TILE;                                    // the tile's first output frame
        const uint32_t nm = tk.out - m0 < TILE ? (uint32_t)(tk.out - m0) : TILE;    // ... and how many it has
        const uint32_t tile_blocks = (nm + UP - 1) / UP;
        const uint32_t nb = PAIRS / ch;     // blocks of a chunk
        const uint32_t e0 = start_of(tk.b);
        const int32_t *in_s = pcm + di.off;
        int32_t *out_s = out + dn.off;
        // the lane's pair: block kb of the chunk, channel c
        const uint32_t kb = div_small(lane, ch, inv), c = lane - kb * ch;
        uint64_t cnt_lo = 0, cnt_hi = 0;
        for (uint32_t kb0 = 0; kb0 < tile_blocks; kb0 += nb) {
            const uint32_t nblk = tile_blocks - kb0 < nb ? tile_blocks - kb0 : nb;  // blocks of the chunk
            const uint32_t np = nblk * ch;                                          // ... and its pairs
            // region index of the first staged frame of the chunk's block 0
            const int64_t j0 = tk.rel + (int64_t)DOWN * ((int64_t)ti * PAIRS + kb0);
            // ---- stage: frame i of the span of pair (k, c) -> s_buf[(k * ch + c) * SPAN + i], zero where the region
            //      does not hold it
            if (IN_PLANAR) {
#pragma unroll 8
                for (uint32_t e = t; e < np * SPAN; e += THREADS) {
                    const uint32_t pr = e / SPAN, i = e - pr * SPAN;
                    const uint32_t k = div_small(pr, ch, inv), cc = pr - k * ch;
                    const int64_t j = j0 + (int64_t)(DOWN * k + i);
                    int32_t v = 0;
                    if (j >= 0 && j < (int64_t)di.frames)
                        v = in_s[(uint64_t)cc * di.stride + (uint64_t)j];
                    s_buf[e] = (uint32_t)v;
                }
            } else {
                // a block's span is one run of SPAN * ch dwords
#pragma unroll 8
                for (uint32_t e = t; e < np * SPAN; e += THREADS) {
                    const uint32_t f = div_small(e, ch, inv), cc = e - f * ch;
                    const uint32_t k = f / SPAN, i = f - k * SPAN;
                    const int64_t j = j0 + (int64_t)(DOWN * k + i);
                    int32_t v = 0;
                    if (j >= 0 && j < (int64_t)di.frames)
                        v = in_s[(uint64_t)j * ch + cc];
                    s_buf[(k * ch + cc) * SPAN + i] = (uint32_t)v;
                }
            }
            __syncthreads();
            // ---- taps: the wave's item is the residues r .. r + R - 1 of every pair, one pair per lane
            for (uint32_t gi = wave; gi < GROUPS; gi += WAVES) {
                const uint32_t r = R * gi;
                const int32_t *row[R];
                uint32_t start0 = 0;
#pragma unroll
                for (uint32_t k = 0; k < R; k++) {
                    // output r + k of a block is residue (b + r + k) mod 147 of the track's grid, and behind the
                    // wrap its window is another 160 frames on
                    const uint32_t sum = tk.b + r + k, wrap = sum >= UP ? 1u : 0u, res = sum - wrap * UP;
                    const uint32_t start = DOWN * wrap + start_of(res) - e0;        // in the block's staged span
                    if (k == 0)
                        start0 = start;
                    const uint32_t shift = __builtin_amdgcn_readfirstlane(start - start0 - k);
                    row[k] = row_of(__builtin_amdgcn_readfirstlane(phase_of(res)), shift);
                }
                if (lane >= np)
                    continue;
                const int32_t *win = reinterpret_cast<const int32_t *>(s_buf) + lane * SPAN + start0;
                int64_t acc[R];
#pragma unroll
                for (uint32_t k = 0; k < R; k++)
                    acc[k] = 0;
                accumulate<R>(acc, row, [&](uint32_t j) { return win[j]; });
                const uint32_t o = UP * (kb0 + kb) + r;                 // the item's first output frame in the tile
                uint32_t cl = 0;
#pragma unroll
                for (uint32_t k = 0; k < R; k++) {
                    uint32_t one = 0;
                    const int32_t y = finish(acc[k], bits, &one);
                    if (o + k < nm) {                                   // (behind the stream's end: not an output)
                        cl += one;
                        if (OUT_PLANAR)
                            out_s[(uint64_t)c * dn.stride + m0 + o + k] = y;
                        else
                            out_s[(m0 + o + k) * ch + c] = y;
                    }
                }
                const uint64_t add = (uint64_t)cl << (16u * (c & 3u));
                cnt_lo += c < 4 ? add : 0ull;
                cnt_hi += c < 4 ? 0ull : add;
            }
            __syncthreads();            // (s_buf has been read: the next chunk fills it)
        }
        cnt_lo = pcmt::block_fold(cnt_lo, s_red, pcmt::FoldSum());
        cnt_hi = pcmt::block_fold(cnt_hi, s_red, pcmt::FoldSum());
        if (t == 0) {
            uint32_t *o = rec + (uint64_t)b * REC;
#pragma unroll
            for (uint32_t cc = 0; cc < 4; cc++) {
                o[cc] = (uint32_t)(cnt_lo >> (16u * cc)) & 0xFFFFu;
                o[4 + cc] = (uint32_t)(cnt_hi >> (16u * cc)) & 0xFFFFu;
            }
        }
    }
}

// ---- step 4: one workgroup per stream sums the stream's records.  A stream whose tiles do not all lie inside the
//      caller's bound is reported as zeros, as one that is not taken.
__global__ __launch_bounds__(THREADS) void k_rs_join(const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                     const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                     const dvda_pcm_decim_piece *__restrict__ piece, uint32_t n,
                                                     const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                     uint32_t max_tiles, dvda_pcm_decim_report *__restrict__ out)
{
    __shared__ uint64_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    const Take tk = take(desc_in[s], desc_out[s], piece ? piece + s : nullptr);
    const uint32_t first = base[s], n_t = tiles_of(tk.out);
    const bool taken = tk.taken && (uint64_t)first + n_t <= max_tiles;
    if (threadIdx.x == 0) {
        out[s].frames_in = taken ? tk.own : 0ull;
        out[s].frames_out = taken ? tk.out : 0ull;
    }
    pcmw::join_clipped(rec, first, taken ? n_t : 0u, taken ? desc_in[s].channels : 0u, s_red, out[s].clipped);
}

} // namespace rsm
