// pcm_compare.h -- the compare of two buffers of decoded PCM, on the device, each side in either int32 layout
// (include/dvda_mlp_hip.h states the contract: per stream pair the frames that differ -- how many, the first, the last,
// in how many runs -- and per channel the values that differ and the largest |a - b|).  All of it is exact.
//
//   tiles   a pair is cut into tiles of TILE frames ALIGNED TO ITS START over its `compared` = min(frames) frames (the
//           last tile of a pair is the ragged one); frames behind `compared` are never read
//   chunk   what a workgroup has in hand at a time: CF frames of the tile, a multiple of the workgroup's size.  A
//           frame-major side is STAGED: the chunk's values, one run of consecutive int32, go to LDS through 16-byte
//           groups aligned in MEMORY (one 16-byte load and one 16-byte LDS store per group; the group that holds the run's
//           first values and the one that holds its last ones value by value, only what is inside) -- every line is
//           fetched once, whatever the channel count.  CF is as many frames as STAGE_WORDS hold.  A planar side is read
//           where it lies: consecutive lanes take consecutive frames of a plane, a wave's load is 256 consecutive bytes.
//   frame   thread t takes frames t, t + THREADS, ... of the chunk and, of each, all channels: the channel loop is
//           unrolled to MAX_CHANNELS with a uniform guard, so a channel's two accumulators are registers named at compile
//           time.  The wave's __ballot of "this frame differs" is a word of the tile's bitmap (64 words of 64 bits, in LDS).
//   bitmap  wave 0 derives what is per frame: lane i takes word i with the top bit of word i - 1 as carry -- count =
//           popcounts, first / last from ffs / clz folded by min / max, runs = popc(m & ~((m << 1) | carry)), the two
//           edge bits.  Frames of the ragged tile behind `compared` are zero bits.
//   tile    one record: first | end | count | runs and the edge bits | per channel differing values, max |a - b|.
//           Every word a join reads was stored by this launch: the workspace need not be cleared.  No atomics.
//   join    one workgroup per pair folds the pair's records, thread j taking tiles j, j + THREADS, ...; runs = the sum
//           of the tiles' runs - the neighbouring tiles of which the earlier one's last frame and the later one's first
//           frame both differ (a look at the neighbour's record: the order of the fold does not matter)
//
// tests/compare_model.py restates all of it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_tiles.h"

namespace cmp {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;

constexpr uint32_t TILE = DVDA_CMP_TILE_FRAMES;
constexpr uint32_t TILE_BLOCKS = 2048;      // workgroups of k_cmp_tiles at most (8 per CU): they stride over the tile list
constexpr uint32_t REC = 4 + 2 * MAX_CHANNELS;      // words of a tile's record
constexpr uint32_t NONE = 0xFFFFFFFFu;      // "no differing frame" as a first index
constexpr uint32_t MAP_WORDS = TILE / 64;   // the tile's bitmap
constexpr uint32_t STAGE_WORDS = TILE;      // values of a staged chunk (16 KiB a side): TILE frames of one channel, ...
constexpr uint32_t HEAD = 1u << 30, TAIL = 1u << 31;        // record word 3: the tile's first / last frame differs
static_assert(MAP_WORDS == 64 && TILE % THREADS == 0, "one lane of a wave per word of the bitmap");
static_assert((STAGE_WORDS / MAX_CHANNELS) / THREADS >= 1, "a chunk holds a frame per thread at least");

// what a pair compares: nothing (SHAPE) unless both descriptors are taken and agree on the channels
__host__ __device__ __forceinline__ bool shape_differs(const dvda_pcm_crc_desc &a, const dvda_pcm_crc_desc &b)
{
    return PCMT_NOT_TAKEN(a) || PCMT_NOT_TAKEN(b) || a.channels != b.channels;
}

__host__ __device__ __forceinline__ uint64_t compared_frames(const dvda_pcm_crc_desc &a, const dvda_pcm_crc_desc &b)
{
    if (shape_differs(a, b))
        return 0;
    return a.frames < b.frames ? a.frames : b.frames;
}

__host__ __device__ __forceinline__ uint32_t tiles_of(uint64_t frames) { return (uint32_t)((frames + TILE - 1) / TILE); }

// ---- step 1: tiles per pair (the index's exclusive scan runs over them)
__global__ void k_cmp_plan(const dvda_pcm_crc_desc *__restrict__ da, const dvda_pcm_crc_desc *__restrict__ db, uint32_t n,
                           uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = tiles_of(compared_frames(da[i], db[i]));
}

// The run p[0, n) into LDS, value k at s[mis + k]; -> mis, the values of the run's first 16-byte group in front of it.
// Whole groups with one 16-byte load each, thread t the groups t, t + THREADS, ...; the ragged ends by threads 0..7.
__device__ __forceinline__ uint32_t stage(const int32_t *__restrict__ p, uint32_t n, int32_t *__restrict__ s, uint32_t t)
{
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
    const int4 *__restrict__ grp = reinterpret_cast<const int4 *>(p - mis);     // 16-byte aligned
    int4 *__restrict__ s4 = reinterpret_cast<int4 *>(s);
    const uint32_t n_groups = (mis + n + 3u) >> 2;
    const uint32_t g_lo = mis ? 1u : 0u, g_hi = (mis + n) >> 2;                 // whole groups: [g_lo, g_hi)
#pragma unroll 4
    for (uint32_t g = g_lo + t; g < g_hi; g += THREADS)
        s4[g] = grp[g];
    if (t < 4) {                            // the group the run starts inside
        if (mis && t >= mis && t - mis < n)
            s[t] = p[t - mis];
    } else if (t < 8) {                     // the group the run ends inside (unless it is the one above)
        const uint32_t k = 4u * g_hi + (t - 4u) - mis;
        if (g_hi >= g_lo && g_hi < n_groups && k < n)
            s[4u * g_hi + (t - 4u)] = p[k];
    }
    return mis;
}

// a value as it would be written at the nominal depth: (v & mask) - (v < 0 ? half : 0); bits == 0: mask all ones, half 0
__device__ __forceinline__ int32_t written(int32_t v, uint32_t mask, uint32_t half)
{
    return (int32_t)(((uint32_t)v & mask) - ((uint32_t)(v >> 31) & half));
}

// a channel's pair of figures in one word for the fold: differing values (at most TILE) | max |a - b| << 32
struct FoldCountMax {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const
    {
        const uint64_t mx = (a >> 32) > (b >> 32) ? (a >> 32) : (b >> 32);
        return mx << 32 | (uint32_t)((uint32_t)a + (uint32_t)b);
    }
    __device__ __forceinline__ uint64_t start(uint64_t) const { return 0ull; }
};

// ---- step 3: the record of every tile.  The workgroups stride over the flat tile list (as many of it as the caller's
//      bound holds: rec has max_tiles records).
template <bool A_PLANAR, bool B_PLANAR>
__global__ __launch_bounds__(THREADS) void k_cmp_tiles(const int32_t *__restrict__ pcm_a,
                                                       const dvda_pcm_crc_desc *__restrict__ desc_a,
                                                       const int32_t *__restrict__ pcm_b,
                                                       const dvda_pcm_crc_desc *__restrict__ desc_b, uint32_t n, uint32_t bits,
                                                       const uint32_t *__restrict__ base, uint32_t *__restrict__ rec,
                                                       uint32_t max_tiles)
{
    __shared__ __attribute__((aligned(16))) int32_t s_a[A_PLANAR ? 4 : STAGE_WORDS + 4];
    __shared__ __attribute__((aligned(16))) int32_t s_b[B_PLANAR ? 4 : STAGE_WORDS + 4];
    __shared__ uint64_t s_map[MAP_WORDS];
    __shared__ uint64_t s_red[WAVES];
    const uint32_t half = bits ? 1u << (bits - 1) : 0u, mask = bits ? half - 1u : 0xFFFFFFFFu;
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc da = desc_a[s], db = desc_b[s];
        const uint32_t ch = da.channels;                            // (a pair that has tiles has 1..8 channels on both sides)
        const uint64_t frames = da.frames < db.frames ? da.frames : db.frames;
        const uint64_t f0 = (uint64_t)(b - base[s]) * TILE;
        const uint32_t nf = frames - f0 < TILE ? (uint32_t)(frames - f0) : TILE;
        const int32_t *__restrict__ pa = pcm_a + da.off + (A_PLANAR ? f0 : f0 * ch);
        const int32_t *__restrict__ pb = pcm_b + db.off + (B_PLANAR ? f0 : f0 * ch);
        // frames of a chunk: what the staging buffers hold, in whole turns of the workgroup
        const uint32_t CF = (A_PLANAR && B_PLANAR) ? TILE : (STAGE_WORDS / ch) & ~(THREADS - 1u);
        uint32_t cnt[MAX_CHANNELS], mx[MAX_CHANNELS];
#pragma unroll
        for (uint32_t c = 0; c < MAX_CHANNELS; c++)
            cnt[c] = mx[c] = 0u;
        __syncthreads();                    // (s_map of the tile before has been read)
        if (t < MAP_WORDS)
            s_map[t] = 0ull;
        for (uint32_t cf = 0; cf < nf; cf += CF) {
            const uint32_t ncf = nf - cf < CF ? nf - cf : CF;
            uint32_t mis_a = 0, mis_b = 0;
            __syncthreads();                // (the chunk before has been read; the bitmap is clear)
            if (!A_PLANAR)
                mis_a = stage(pa + (uint64_t)cf * ch, ncf * ch, s_a, t);
            if (!B_PLANAR)
                mis_b = stage(pb + (uint64_t)cf * ch, ncf * ch, s_b, t);
            if (!A_PLANAR || !B_PLANAR)
                __syncthreads();
            for (uint32_t j0 = 0; j0 < ncf; j0 += THREADS) {
                const uint32_t fl = j0 + t;                         // frame of the chunk
                const bool on = fl < ncf;
                int32_t va[MAX_CHANNELS], vb[MAX_CHANNELS];
#pragma unroll
                for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
                    va[c] = vb[c] = 0;
                    if (on && c < ch) {
                        va[c] = A_PLANAR ? pa[(uint64_t)c * da.stride + cf + fl] : s_a[mis_a + fl * ch + c];
                        vb[c] = B_PLANAR ? pb[(uint64_t)c * db.stride + cf + fl] : s_b[mis_b + fl * ch + c];
                    }
                }
                bool any = false;
#pragma unroll
                for (uint32_t c = 0; c < MAX_CHANNELS; c++) {       // (a channel that is not there: 0 against 0)
                    const int32_t x = written(va[c], mask, half), y = written(vb[c], mask, half);
                    const uint32_t d = x > y ? (uint32_t)x - (uint32_t)y : (uint32_t)y - (uint32_t)x;
                    cnt[c] += d ? 1u : 0u;
                    mx[c] = d > mx[c] ? d : mx[c];
                    any |= d != 0u;
                }
                const uint64_t m = __ballot(any);
                if (lane == 0)
                    s_map[((cf + j0) >> 6) + wave] = m;
            }
        }
        // per channel, over the workgroup (the first fold's barriers also publish the bitmap)
        uint64_t per[MAX_CHANNELS];
#pragma unroll
        for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
            per[c] = 0ull;
            if (c < ch)
                per[c] = pcmt::block_fold((uint64_t)mx[c] << 32 | cnt[c], s_red, FoldCountMax());
        }
        // per frame, from the bitmap: wave 0, lane i word i
        if (wave == 0) {
            const uint64_t m = s_map[lane];
            const uint64_t carry = lane ? s_map[lane - 1] >> 63 : 0ull;
            uint32_t count = (uint32_t)__popcll(m);
            uint32_t runs = (uint32_t)__popcll(m & ~(m << 1 | carry));
            uint32_t first = m ? lane * 64u + (uint32_t)__ffsll((long long)m) - 1u : NONE;
            uint32_t end = m ? lane * 64u + 64u - (uint32_t)__clzll((long long)m) : 0u;
            for (int o = 32; o; o >>= 1) {
                count += __shfl_xor(count, o, 64);
                runs += __shfl_xor(runs, o, 64);
                const uint32_t f = __shfl_xor(first, o, 64), e = __shfl_xor(end, o, 64);
                first = f < first ? f : first;
                end = e > end ? e : end;
            }
            if (lane == 0) {
                const uint32_t head = (uint32_t)(s_map[0] & 1u);
                const uint32_t tail = (uint32_t)(s_map[(nf - 1u) >> 6] >> ((nf - 1u) & 63u)) & 1u;
                uint32_t *out = rec + (uint64_t)b * REC;
                out[0] = first;
                out[1] = end;
                out[2] = count;
                out[3] = runs | (head ? HEAD : 0u) | (tail ? TAIL : 0u);
#pragma unroll
                for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
                    out[4 + 2 * c] = (uint32_t)per[c];
                    out[5 + 2 * c] = (uint32_t)(per[c] >> 32);
                }
            }
        }
    }
}

// ---- step 4: one workgroup per pair joins the pair's records.  A pair whose tiles do not all lie inside the caller's
//      bound is reported as zeros.
__global__ __launch_bounds__(THREADS) void k_cmp_join(const dvda_pcm_crc_desc *__restrict__ desc_a,
                                                      const dvda_pcm_crc_desc *__restrict__ desc_b, uint32_t n,
                                                      const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                      uint32_t max_tiles, dvda_pcm_diff *__restrict__ out)
{
    __shared__ uint64_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    const dvda_pcm_crc_desc da = desc_a[s], db = desc_b[s];
    const bool shape = shape_differs(da, db);
    const uint64_t compared = compared_frames(da, db);
    const uint32_t first_tile = base[s], n_t = tiles_of(compared);
    const bool inside = (uint64_t)first_tile + n_t <= max_tiles;
    const uint32_t ch = shape || !inside ? 0u : da.channels, turns = inside ? n_t : 0u;
    const uint32_t *r0 = rec + (uint64_t)first_tile * REC;
    // first as a minimum, end as the minimum of the complement; a seam: this tile's first and the one before's last differ
    uint64_t first = compared, not_end = ~0ull, count = 0, runs = 0, seams = 0;
    for (uint32_t i = threadIdx.x; i < turns; i += THREADS) {
        const uint32_t *r = r0 + (uint64_t)i * REC;
        const uint32_t f = r[0], e = r[1], w = r[3];
        if (f != NONE && (uint64_t)i * TILE + f < first)
            first = (uint64_t)i * TILE + f;
        if (e && ~((uint64_t)i * TILE + e) < not_end)
            not_end = ~((uint64_t)i * TILE + e);
        count += r[2];
        runs += w & ~(HEAD | TAIL);
        if (i && (w & HEAD) && (r[3 - (int)REC] & TAIL))
            seams++;
    }
    first = pcmt::block_fold(first, s_red, pcmt::FoldMin());
    not_end = pcmt::block_fold(not_end, s_red, pcmt::FoldMin());
    count = pcmt::block_fold(count, s_red, pcmt::FoldSum());
    runs = pcmt::block_fold(runs, s_red, pcmt::FoldSum());
    seams = pcmt::block_fold(seams, s_red, pcmt::FoldSum());
    if (threadIdx.x == 0) {
        dvda_pcm_diff &o = out[s];
        o.frames_a = !inside || PCMT_NOT_TAKEN(da) ? 0ull : da.frames;
        o.frames_b = !inside || PCMT_NOT_TAKEN(db) ? 0ull : db.frames;
        o.compared = inside ? compared : 0ull;
        o.diff_frames = count;
        o.first_diff = inside ? first : 0ull;
        o.diff_end = ~not_end;
        o.runs = runs - seams;
        o.channels = ch;
        o.flags = inside && shape ? DVDA_CMP_SHAPE : 0u;
    }
    for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
        uint64_t values = 0, not_max = 0xFFFFFFFFull;
        if (c < ch)
            for (uint32_t i = threadIdx.x; i < turns; i += THREADS) {
                const uint32_t *r = r0 + (uint64_t)i * REC + 4 + 2 * c;
                const uint32_t z = ~r[1];
                values += r[0];
                not_max = z < not_max ? z : not_max;
            }
        values = pcmt::block_fold(values, s_red, pcmt::FoldSum());
        not_max = pcmt::block_fold(not_max, s_red, pcmt::FoldMin());
        if (threadIdx.x == 0) {
            out[s].diff_values[c] = c < ch ? values : 0ull;
            out[s].max_abs[c] = c < ch ? ~(uint32_t)not_max : 0u;
        }
    }
}

} // namespace cmp
