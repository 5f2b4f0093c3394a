// pcm_levels.h -- the level report of decoded PCM, on the device, from either int32 layout the decode wrote
// (include/dvda_mlp_hip.h states the contract: per channel min, max, exact sum and the values outside the nominal
// range; per stream the frames of digital silence at both ends).  All of it is exact integer arithmetic.
//
//   tiles  a stream is cut into tiles of TILE frames ALIGNED TO ITS START (the last tile of a stream is the ragged one)
//   run    what a workgroup streams: `n` consecutive int32 values -- one channel's frames of the tile (planar: a run per
//          channel) or all of the tile's values (frame-major: one run).  The run is covered by 16-byte groups aligned in
//          MEMORY; thread t takes groups t, t + S, t + 2 S, ... with one 16-byte load each (coalesced), the group that
//          holds the run's first values and the one that holds its last ones value by value (only what is inside).
//   slots  a thread keeps four accumulators, one per position in a group.  Frame-major, S is the largest multiple of
//          the channel count up to the workgroup's size: 4 S values are whole frames, so a thread's position j holds
//          the same channel in every group it takes -- (4 t + j - misalignment) mod channels, computed once per tile by
//          a multiply-high -- and no value needs a division.  Planar, all four belong to the run's channel.
//   silent a thread also keeps the smallest and the largest run index at which it saw a non-zero value
//   tile   per channel the slots of that channel are folded, over the wave by shuffles, over the waves through a few
//          LDS words, and one record per tile is stored: first non-zero frame | last non-zero frame + 1 | per channel
//          min, max, over, sum (two words).  Every word a join reads was stored by this launch: the workspace need
//          not be cleared.  No atomics: the same words whatever ran first.
//   join   one workgroup per stream folds the stream's records, thread j taking tiles j, j + THREADS, ..., and
//          composes lead_silent / trail_silent from the first / last non-zero frame over all tiles
//
// tests/levels_model.py restates all of it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_tiles.h"

namespace lvl {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;

constexpr uint32_t TILE = DVDA_LVL_TILE_FRAMES;
constexpr uint32_t TILE_BLOCKS = 2048;      // workgroups of k_lvl_tiles at most (8 per CU): they stride over the tile list
constexpr uint32_t REC = 2 + 5 * MAX_CHANNELS;     // words of a tile's record
constexpr uint32_t NONE = 0xFFFFFFFFu;      // "no non-zero value" as a first index
constexpr int BATCH = 4;                    // 16-byte loads a thread has in flight
static_assert(TILE % 4 == 0 && TILE * MAX_CHANNELS < (1u << 17), "run indices and the multiply-high stay small");

// PCM frames of a stream (0 for a descriptor outside what the kernels take)
__host__ __device__ __forceinline__ uint64_t stream_frames(const dvda_pcm_crc_desc &d)
{
    if (PCMT_NOT_TAKEN(d))
        return 0;
    return d.frames;
}

__host__ __device__ __forceinline__ uint32_t tiles_of(uint64_t frames) { return (uint32_t)((frames + TILE - 1) / TILE); }

// ---- step 1: tiles per stream (the index's exclusive scan runs over them)
__global__ void k_lvl_plan(const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = tiles_of(stream_frames(desc[i]));
}

struct Slot {
    int32_t mn, mx;
    uint32_t over;
    int64_t sum;
};

__device__ __forceinline__ Slot slot_none() { return Slot{INT32_MAX, INT32_MIN, 0u, 0}; }

// the nominal range as one unsigned compare: v is inside [-half, half - 1] exactly when v + half < 2 * half (mod 2^32)
__device__ __forceinline__ void take(Slot &s, int32_t v, uint32_t half)
{
    s.mn = v < s.mn ? v : s.mn;
    s.mx = v > s.mx ? v : s.mx;
    s.over += ((uint32_t)v + half >= 2u * half) ? 1u : 0u;
    s.sum += v;
}

__device__ __forceinline__ void fold(Slot &s, const Slot &o)
{
    s.mn = o.mn < s.mn ? o.mn : s.mn;
    s.mx = o.mx > s.mx ? o.mx : s.mx;
    s.over += o.over;
    s.sum += o.sum;
}

__device__ __forceinline__ void wave_fold(Slot &s)
{
    for (int o = 32; o; o >>= 1) {
        Slot r;
        r.mn = __shfl_xor(s.mn, o, 64);
        r.mx = __shfl_xor(s.mx, o, 64);
        r.over = __shfl_xor(s.over, o, 64);
        r.sum = __shfl_xor((long long)s.sum, o, 64);
        fold(s, r);
    }
}

// one whole group at run index k0 (>= 0): its four values into the four slots
__device__ __forceinline__ void take_group(Slot (&a)[4], const int4 q, uint32_t k0, uint32_t half, uint32_t &first,
                                           uint32_t &last1)
{
    take(a[0], q.x, half);
    take(a[1], q.y, half);
    take(a[2], q.z, half);
    take(a[3], q.w, half);
    const bool any = (q.x | q.y | q.z | q.w) != 0;
    const uint32_t lo = q.x ? 0u : q.y ? 1u : q.z ? 2u : 3u;
    const uint32_t hi = q.w ? 4u : q.z ? 3u : q.y ? 2u : 1u;
    first = min(first, any ? k0 + lo : NONE);
    last1 = max(last1, any ? k0 + hi : 0u);
}

// a group that holds an end of the run: the values inside [0, n), one by one -- nothing outside the run is read
__device__ __forceinline__ void take_edge(Slot (&a)[4], const int32_t *__restrict__ p, uint32_t n, int32_t k0, uint32_t half,
                                          uint32_t &first, uint32_t &last1)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int32_t k = k0 + j;
        if (k >= 0 && (uint32_t)k < n) {
            const int32_t v = p[k];
            take(a[j], v, half);
            if (v) {
                first = (uint32_t)k < first ? (uint32_t)k : first;
                last1 = (uint32_t)k + 1u > last1 ? (uint32_t)k + 1u : last1;
            }
        }
    }
}

// The run p[0, n) into thread t's slots (t < S; S: groups between two of a thread's).  first / last1: smallest run index
// of a non-zero value / largest + 1 this thread has seen, carried from run to run.
__device__ __forceinline__ void scan_run(const int32_t *__restrict__ p, uint32_t n, uint32_t S, uint32_t t, uint32_t half,
                                         Slot (&a)[4], uint32_t &first, uint32_t &last1)
{
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;  // values of the first group in front of the run
    const int4 *__restrict__ grp = reinterpret_cast<const int4 *>(p - mis);     // 16-byte aligned
    const uint32_t n_groups = (mis + n + 3u) >> 2;
    const uint32_t g_lo = mis ? 1u : 0u, g_hi = (mis + n) >> 2;                 // whole groups: [g_lo, g_hi)
    uint32_t g = t;
    if (g < g_lo) {                                                             // (thread 0, a run that starts inside a group)
        take_edge(a, p, n, -(int32_t)mis, half, first, last1);
        g += S;
    }
    for (; g + (BATCH - 1) * S < g_hi; g += BATCH * S) {
        int4 q[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; i++)
            q[i] = grp[g + i * S];
#pragma unroll
        for (int i = 0; i < BATCH; i++)
            take_group(a, q[i], 4u * (g + i * S) - mis, half, first, last1);
    }
    for (; g < g_hi; g += S)
        take_group(a, grp[g], 4u * g - mis, half, first, last1);
    if (g < n_groups && g >= g_lo)                                              // the run ends inside this group
        take_edge(a, p, n, (int32_t)(4u * g) - (int32_t)mis, half, first, last1);
}

// ---- step 3: the record of every tile.  The workgroups stride over the flat tile list (as many of it as the caller's
//      bound holds: rec has max_tiles records).
template <bool PLANAR>
__global__ __launch_bounds__(THREADS, PLANAR ? 7 : 8) void k_lvl_tiles(const int32_t *__restrict__ pcm,
                                                       const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t bits,
                                                       const uint32_t *__restrict__ base, uint32_t *__restrict__ rec,
                                                       uint32_t max_tiles)
{
    __shared__ uint32_t s_rec[WAVES][REC];
    const uint32_t half = 1u << (bits - 1);
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc d = desc[s];
        const uint32_t ch = d.channels;
        const uint64_t f0 = (uint64_t)(b - base[s]) * TILE;         // (a stream that has tiles has frames and 1..8 channels)
        const uint32_t nf = d.frames - f0 < TILE ? (uint32_t)(d.frames - f0) : TILE;
        uint32_t first = NONE, last1 = 0;
        __syncthreads();                    // (s_rec of the tile before has been read)
        if (PLANAR) {
            for (uint32_t c = 0; c < ch; c++) {
                Slot a[4] = {slot_none(), slot_none(), slot_none(), slot_none()};
                scan_run(pcm + d.off + (uint64_t)c * d.stride + f0, nf, THREADS, t, half, a, first, last1);
                fold(a[0], a[1]);
                fold(a[2], a[3]);
                fold(a[0], a[2]);
                wave_fold(a[0]);
                if (lane == 0) {
                    uint32_t *o = &s_rec[wave][2 + 5 * c];
                    o[0] = (uint32_t)a[0].mn;
                    o[1] = (uint32_t)a[0].mx;
                    o[2] = a[0].over;
                    o[3] = (uint32_t)a[0].sum;
                    o[4] = (uint32_t)((uint64_t)a[0].sum >> 32);
                }
            }
        } else {
            const uint32_t S = THREADS - THREADS % ch;              // 4 S values are whole frames
            const int32_t *p = pcm + d.off + f0 * ch;
            Slot a[4] = {slot_none(), slot_none(), slot_none(), slot_none()};
            if (t < S)
                scan_run(p, nf * ch, S, t, half, a, first, last1);
            // the channel of slot j: (4 t + j - mis) mod ch, through y / ch = umulhi(y, magic) (y < 2^17, ch in 2..8)
            const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
            const uint32_t magic = 0xFFFFFFFFu / ch + 1u;
            uint32_t cj[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t y = 4u * t + 4u * S + (uint32_t)j - mis;
                cj[j] = ch == 1 ? 0u : y - __umulhi(y, magic) * ch;
            }
            for (uint32_t c = 0; c < ch; c++) {
                Slot r = slot_none();
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (cj[j] == c)
                        fold(r, a[j]);
                wave_fold(r);
                if (lane == 0) {
                    uint32_t *o = &s_rec[wave][2 + 5 * c];
                    o[0] = (uint32_t)r.mn;
                    o[1] = (uint32_t)r.mx;
                    o[2] = r.over;
                    o[3] = (uint32_t)r.sum;
                    o[4] = (uint32_t)((uint64_t)r.sum >> 32);
                }
            }
        }
        for (int o = 32; o; o >>= 1) {
            const uint32_t f = __shfl_xor(first, o, 64), l = __shfl_xor(last1, o, 64);
            first = f < first ? f : first;
            last1 = l > last1 ? l : last1;
        }
        if (lane == 0) {
            s_rec[wave][0] = first;
            s_rec[wave][1] = last1;
        }
        __syncthreads();
        uint32_t *out = rec + (uint64_t)b * REC;
        if (t < ch) {
            Slot r = slot_none();
            for (int w = 0; w < WAVES; w++) {
                const uint32_t *i = &s_rec[w][2 + 5 * t];
                Slot x;
                x.mn = (int32_t)i[0];
                x.mx = (int32_t)i[1];
                x.over = i[2];
                x.sum = (int64_t)((uint64_t)i[3] | (uint64_t)i[4] << 32);
                fold(r, x);
            }
            out[2 + 5 * t] = (uint32_t)r.mn;
            out[3 + 5 * t] = (uint32_t)r.mx;
            out[4 + 5 * t] = r.over;
            out[5 + 5 * t] = (uint32_t)r.sum;
            out[6 + 5 * t] = (uint32_t)((uint64_t)r.sum >> 32);
        } else if (t == MAX_CHANNELS) {
            uint32_t f = NONE, l = 0;
            for (int w = 0; w < WAVES; w++) {
                f = s_rec[w][0] < f ? s_rec[w][0] : f;
                l = s_rec[w][1] > l ? s_rec[w][1] : l;
            }
            if (!PLANAR) {                  // run indices -> frames of the tile
                f = f == NONE ? NONE : f / ch;
                l = l ? (l - 1u) / ch + 1u : 0u;
            }
            out[0] = f;
            out[1] = l;
        }
    }
}

// ---- step 4: one workgroup per stream joins the stream's records.  A stream whose tiles do not all lie inside the
//      caller's bound is reported as zeros.
__global__ __launch_bounds__(THREADS) void k_lvl_join(const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n,
                                                      const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                      uint32_t max_tiles, dvda_pcm_levels *__restrict__ out)
{
    __shared__ uint64_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    uint64_t frames = stream_frames(desc[s]);
    const uint32_t first = base[s], n_t = tiles_of(frames);
    if ((uint64_t)first + n_t > max_tiles)
        frames = 0;
    const uint32_t ch = frames ? desc[s].channels : 0u, turns = frames ? n_t : 0u;
    const uint32_t *r0 = rec + (uint64_t)first * REC;
    // silence: the first non-zero frame (none: `frames`) and the last one + 1 (none: 0); max as the min of the complement
    uint64_t lead = frames, not_end = ~0ull;
    for (uint32_t i = threadIdx.x; i < turns; i += THREADS) {
        const uint32_t *r = r0 + (uint64_t)i * REC;
        const uint32_t f = r[0], l = r[1];
        if (f != NONE && (uint64_t)i * TILE + f < lead)
            lead = (uint64_t)i * TILE + f;
        if (l && ~((uint64_t)i * TILE + l) < not_end)
            not_end = ~((uint64_t)i * TILE + l);
    }
    lead = pcmt::block_fold(lead, s_red, pcmt::FoldMin());
    not_end = pcmt::block_fold(not_end, s_red, pcmt::FoldMin());
    if (threadIdx.x == 0) {
        out[s].frames = frames;
        out[s].lead_silent = lead;
        out[s].trail_silent = frames - ~not_end;
    }
    for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
        // min and max as unsigned minima of the order-preserving images v ^ 2^31 and ~(v ^ 2^31)
        uint64_t mn = 0xFFFFFFFFull, not_mx = 0xFFFFFFFFull, over = 0, sum = 0;
        if (c < ch)
            for (uint32_t i = threadIdx.x; i < turns; i += THREADS) {
                const uint32_t *r = r0 + (uint64_t)i * REC + 2 + 5 * c;
                const uint32_t a = r[0] ^ 0x80000000u, z = ~(r[1] ^ 0x80000000u);
                mn = a < mn ? a : mn;
                not_mx = z < not_mx ? z : not_mx;
                over += r[2];
                sum += (uint64_t)r[3] | (uint64_t)r[4] << 32;
            }
        mn = pcmt::block_fold(mn, s_red, pcmt::FoldMin());
        not_mx = pcmt::block_fold(not_mx, s_red, pcmt::FoldMin());
        over = pcmt::block_fold(over, s_red, pcmt::FoldSum());
        sum = pcmt::block_fold(sum, s_red, pcmt::FoldSum());
        if (threadIdx.x == 0) {
            const bool live = c < ch;
            out[s].min[c] = live ? (int32_t)((uint32_t)mn ^ 0x80000000u) : 0;
            out[s].max[c] = live ? (int32_t)(~(uint32_t)not_mx ^ 0x80000000u) : 0;
            out[s].over[c] = live ? over : 0;
            out[s].sum[c] = live ? (int64_t)sum : 0;
        }
    }
}

} // namespace lvl
