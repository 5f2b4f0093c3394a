// pcm_energy.h -- the energy report of decoded PCM, on the device, from either int32 layout the decode wrote
// (include/dvda_mlp_hip.h states the contract: a stream is cut into blocks of B frames on a grid whose first block has
// `lead` frames; per block and channel the exact sum of v * v as 128 bits and the largest |v|).  All of it is exact
// integer arithmetic: a square of an int32 is at most 2^62, 2^40 of them sum to at most 2^102.
//
//   pieces the unit of the flat list (pcm_tiles.h) is a piece: at most PIECE consecutive frames of ONE block.  A block
//          of L frames has ceil(L / PIECE) pieces, so a block shorter than PIECE is one piece and a long block is
//          spread over as many workgroups as it has pieces.  Pieces per stream, and the block and the frames of piece q
//          of a stream, are closed forms of (frames, lead, B): Grid.
//   run    what a workgroup streams, as in pcm_levels.h: `n` consecutive int32 values -- one channel's frames of the
//          piece (planar: a run per channel) or all of the piece's values (frame-major: one run) -- covered by 16-byte
//          groups aligned in MEMORY, thread t taking groups t, t + S, ...; the groups that hold the run's ends value
//          by value, nothing outside the run read.
//   slots  four accumulators per thread, one per position in a group; frame-major, S is the largest multiple of the
//          channel count up to the workgroup's size, so a thread's position j holds one channel in every group it takes
//          and no value needs a division (pcm_levels.h).
//   value  a = |v| as unsigned (2^31 for -2^31); s = a * a; lo += s; hi += lo < s; peak = max(peak, a)
//   fold   per channel, over the wave by shuffles and over the waves through LDS, the sum as limbs that cannot
//          overflow -- bits 0..31, bits 32..63 and the high word of every thread's sum, each added up in 64 bits -- and
//          carried once.  A piece's sum is below 2^74: its record holds 96 bits of it and the peak, four words per
//          channel.  Every word a join reads was stored by this launch: the workspace need not be cleared.  No atomics.
//   join   one workgroup per stream; thread j takes blocks j, j + THREADS, ..., adds each block's pieces (128-bit, with
//          carry) and writes the block's record when j is below the stream's cap
//
// tests/energy_model.py restates all of it with Python integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_tiles.h"

namespace nrg {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;

constexpr uint32_t PIECE = DVDA_NRG_PIECE_FRAMES;
constexpr uint32_t TILE_BLOCKS = 2048;      // workgroups of k_nrg_tiles at most (8 per CU): they stride over the piece list
constexpr uint32_t REC = 4 * MAX_CHANNELS;  // words of a piece's record: per channel sum bits 0..31, 32..63, 64..95, peak
constexpr uint32_t LIMBS = 6;               // words a wave leaves per channel: limb 0, limb 1 (two words each), limb 2, peak
constexpr uint32_t SATURATED = 0x80000000u; // a stream's piece count from here on: outside every bound a caller can give
constexpr int BATCH = 4;                    // 16-byte loads a thread has in flight
static_assert(PIECE % 4 == 0 && PIECE * MAX_CHANNELS < (1u << 17), "run indices and the multiply-high stay small");
static_assert(DVDA_NRG_MIN_BLOCK >= 1 && DVDA_NRG_MAX_BLOCK <= (1u << 24), "a block's frames fit its record");

// ---- the grid of one stream, in closed form
struct Grid {
    uint64_t nfull;         // blocks of B frames behind the first
    uint32_t l0, tail;      // frames of the first block / of the ragged last one (0: there is none)
    uint32_t p0, pb, pt;    // pieces of the first block, of a block of B frames, of the ragged last one
    uint32_t B;

    __host__ __device__ uint64_t blocks() const { return (l0 ? 1u : 0u) + nfull + (tail ? 1u : 0u); }
    __host__ __device__ uint64_t pieces() const { return (uint64_t)p0 + nfull * pb + pt; }
    // block j (< blocks()): its first piece within the stream, its pieces, its frames
    __host__ __device__ void block(uint64_t j, uint64_t *piece, uint32_t *n_pieces, uint32_t *frames) const
    {
        if (j == 0) {
            *piece = 0, *n_pieces = p0, *frames = l0;
        } else {
            *piece = p0 + (j - 1) * pb;
            *n_pieces = j - 1 < nfull ? pb : pt;
            *frames = j - 1 < nfull ? B : tail;
        }
    }
    // piece q (< pieces()): the stream's frame it starts at, its frames
    __host__ __device__ void piece(uint32_t q, uint64_t *f0, uint32_t *nf) const
    {
        uint64_t start = 0;
        uint32_t len = l0, k = q;
        if (q >= p0) {
            const uint32_t jj = (q - p0) / pb;
            k = (q - p0) - jj * pb;
            start = l0 + (uint64_t)jj * B;
            len = jj < nfull ? B : tail;
        }
        *f0 = start + (uint64_t)k * PIECE;
        *nf = len - k * PIECE < PIECE ? len - k * PIECE : PIECE;
    }
};

__host__ __device__ __forceinline__ uint32_t pieces_of(uint32_t len) { return (len + PIECE - 1) / PIECE; }

// (a descriptor outside what the kernels take, or a lead outside 1 .. B: no frames, no blocks)
__host__ __device__ __forceinline__ Grid grid_of(const dvda_pcm_crc_desc &d, uint32_t lead, uint32_t B)
{
    uint64_t frames = d.frames;
    if (PCMT_NOT_TAKEN(d) || lead == 0 || lead > B)
        frames = 0;
    Grid g;
    g.B = B;
    g.l0 = frames < lead ? (uint32_t)frames : lead;
    const uint64_t rest = frames - g.l0;
    g.nfull = rest / B;
    g.tail = (uint32_t)(rest - g.nfull * B);
    g.p0 = pieces_of(g.l0);
    g.pb = pieces_of(B);
    g.pt = pieces_of(g.tail);
    return g;
}

__device__ __forceinline__ uint32_t lead_of(const uint32_t *__restrict__ d_lead, uint32_t s, uint32_t B)
{
    return d_lead ? d_lead[s] : B;
}

// ---- step 1: pieces per stream (the index's exclusive scan runs over them)
__global__ void k_nrg_plan(const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t B,
                           const uint32_t *__restrict__ d_lead, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint64_t p = grid_of(desc[i], lead_of(d_lead, i, B), B).pieces();
        cnt[i] = p < SATURATED ? (uint32_t)p : SATURATED;
    }
}

struct Slot {
    uint64_t lo;
    uint32_t hi, peak;
};

__device__ __forceinline__ Slot slot_none() { return Slot{0ull, 0u, 0u}; }

__device__ __forceinline__ void take(Slot &s, int32_t v)
{
    const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    const uint64_t q = (uint64_t)a * a;
    s.lo += q;
    s.hi += s.lo < q ? 1u : 0u;
    s.peak = a > s.peak ? a : s.peak;
}

__device__ __forceinline__ void fold(Slot &s, const Slot &o)
{
    s.lo += o.lo;
    s.hi += o.hi + (s.lo < o.lo ? 1u : 0u);
    s.peak = o.peak > s.peak ? o.peak : s.peak;
}

// a thread's sum as limbs that a workgroup can add up without a carry: each is below 2^32 and at most 4 * THREADS are added
struct Limbs {
    uint64_t l0, l1;
    uint32_t l2, peak;
};

__device__ __forceinline__ Limbs limbs_of(const Slot &s) { return Limbs{s.lo & 0xFFFFFFFFull, s.lo >> 32, s.hi, s.peak}; }

__device__ __forceinline__ void wave_fold(Limbs &s)
{
    for (int o = 32; o; o >>= 1) {
        s.l0 += (uint64_t)__shfl_xor((unsigned long long)s.l0, o, 64);
        s.l1 += (uint64_t)__shfl_xor((unsigned long long)s.l1, o, 64);
        s.l2 += __shfl_xor(s.l2, o, 64);
        const uint32_t p = __shfl_xor(s.peak, o, 64);
        s.peak = p > s.peak ? p : s.peak;
    }
}

__device__ __forceinline__ void put_limbs(uint32_t *o, const Limbs &s)
{
    o[0] = (uint32_t)s.l0;
    o[1] = (uint32_t)(s.l0 >> 32);
    o[2] = (uint32_t)s.l1;
    o[3] = (uint32_t)(s.l1 >> 32);
    o[4] = s.l2;
    o[5] = s.peak;
}

__device__ __forceinline__ void take_group(Slot (&a)[4], const int4 q)
{
    take(a[0], q.x);
    take(a[1], q.y);
    take(a[2], q.z);
    take(a[3], q.w);
}

// a group that holds an end of the run: the values inside [0, n), one by one -- nothing outside the run is read
__device__ __forceinline__ void take_edge(Slot (&a)[4], const int32_t *__restrict__ p, uint32_t n, int32_t k0)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int32_t k = k0 + j;
        if (k >= 0 && (uint32_t)k < n)
            take(a[j], p[k]);
    }
}

// The run p[0, n) into thread t's slots (t < S; S: groups between two of a thread's): the walk of lvl::scan_run.
__device__ __forceinline__ void scan_run(const int32_t *__restrict__ p, uint32_t n, uint32_t S, uint32_t t, Slot (&a)[4])
{
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;  // values of the first group in front of the run
    const int4 *__restrict__ grp = reinterpret_cast<const int4 *>(p - mis);     // 16-byte aligned
    const uint32_t n_groups = (mis + n + 3u) >> 2;
    const uint32_t g_lo = mis ? 1u : 0u, g_hi = (mis + n) >> 2;                 // whole groups: [g_lo, g_hi)
    uint32_t g = t;
    if (g < g_lo) {                                                             // (thread 0, a run that starts inside a group)
        take_edge(a, p, n, -(int32_t)mis);
        g += S;
    }
    for (; g + (BATCH - 1) * S < g_hi; g += BATCH * S) {
        int4 q[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; i++)
            q[i] = grp[g + i * S];
#pragma unroll
        for (int i = 0; i < BATCH; i++)
            take_group(a, q[i]);
    }
    for (; g < g_hi; g += S)
        take_group(a, grp[g]);
    if (g < n_groups && g >= g_lo)                                              // the run ends inside this group
        take_edge(a, p, n, (int32_t)(4u * g) - (int32_t)mis);
}

// ---- step 3: the record of every piece.  The workgroups stride over the flat piece list (as many of it as the caller's
//      bound holds: rec has max_tiles records).
template <bool PLANAR>
__global__ __launch_bounds__(THREADS, PLANAR ? 7 : 8) void k_nrg_tiles(const int32_t *__restrict__ pcm,
                                                       const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t B,
                                                       const uint32_t *__restrict__ d_lead,
                                                       const uint32_t *__restrict__ base, uint32_t *__restrict__ rec,
                                                       uint32_t max_tiles)
{
    __shared__ uint32_t s_rec[WAVES][LIMBS * MAX_CHANNELS];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc d = desc[s];
        const Grid g = grid_of(d, lead_of(d_lead, s, B), B);
        const uint32_t q = b - base[s];
        if (q >= g.pieces())                // (counts that wrapped the scan: no piece of this stream, nothing is read)
            continue;
        const uint32_t ch = d.channels;
        uint64_t f0;
        uint32_t nf;
        g.piece(q, &f0, &nf);
        __syncthreads();                    // (s_rec of the piece before has been read)
        if (PLANAR) {
            for (uint32_t c = 0; c < ch; c++) {
                Slot a[4] = {slot_none(), slot_none(), slot_none(), slot_none()};
                scan_run(pcm + d.off + (uint64_t)c * d.stride + f0, nf, THREADS, t, a);
                fold(a[0], a[1]);
                fold(a[2], a[3]);
                fold(a[0], a[2]);
                Limbs r = limbs_of(a[0]);
                wave_fold(r);
                if (lane == 0)
                    put_limbs(&s_rec[wave][LIMBS * c], r);
            }
        } else {
            const uint32_t S = THREADS - THREADS % ch;              // 4 S values are whole frames
            const int32_t *p = pcm + d.off + f0 * ch;
            Slot a[4] = {slot_none(), slot_none(), slot_none(), slot_none()};
            if (t < S)
                scan_run(p, nf * ch, S, t, a);
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
                Slot x = slot_none();
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (cj[j] == c)
                        fold(x, a[j]);
                Limbs r = limbs_of(x);
                wave_fold(r);
                if (lane == 0)
                    put_limbs(&s_rec[wave][LIMBS * c], r);
            }
        }
        __syncthreads();
        if (t < ch) {
            uint64_t l0 = 0, l1 = 0;
            uint32_t l2 = 0, peak = 0;
            for (int w = 0; w < WAVES; w++) {
                const uint32_t *i = &s_rec[w][LIMBS * t];
                l0 += (uint64_t)i[0] | (uint64_t)i[1] << 32;
                l1 += (uint64_t)i[2] | (uint64_t)i[3] << 32;
                l2 += i[4];
                peak = i[5] > peak ? i[5] : peak;
            }
            // the one carry: l0 + l1 * 2^32 + l2 * 2^64, below 2^74
            const uint64_t lo = l0 + (l1 << 32);
            const uint32_t hi = l2 + (uint32_t)(l1 >> 32) + (lo < l0 ? 1u : 0u);
            uint32_t *out = rec + (uint64_t)b * REC + 4 * t;
            out[0] = (uint32_t)lo;
            out[1] = (uint32_t)(lo >> 32);
            out[2] = hi;
            out[3] = peak;
        }
    }
}

// ---- step 4: one workgroup per stream adds up the pieces of every block.  A stream whose pieces do not all lie inside
//      the caller's bound has no blocks.  Blocks at and behind the stream's cap are counted and not written.
__global__ __launch_bounds__(THREADS) void k_nrg_join(const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t B,
                                                      const uint32_t *__restrict__ d_lead,
                                                      const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                      uint32_t max_tiles, dvda_pcm_energy_block *__restrict__ blocks,
                                                      const uint64_t *__restrict__ block_off,
                                                      const uint64_t *__restrict__ block_cap, uint64_t *__restrict__ nblocks)
{
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    const Grid g = grid_of(desc[s], lead_of(d_lead, s, B), B);
    const uint32_t first = base[s];
    uint64_t nb = g.blocks();
    if ((uint64_t)first + g.pieces() > max_tiles)
        nb = 0;
    if (threadIdx.x == 0)
        nblocks[s] = nb;
    const uint32_t ch = desc[s].channels;           // (1..8 when the stream has blocks)
    const uint64_t cap = block_cap[s], todo = nb < cap ? nb : cap;
    dvda_pcm_energy_block *out = blocks + block_off[s];
    for (uint64_t j = threadIdx.x; j < todo; j += THREADS) {
        uint64_t p;
        uint32_t np, frames;
        g.block(j, &p, &np, &frames);
        const uint32_t *r0 = rec + ((uint64_t)first + p) * REC;
        dvda_pcm_energy_block *o = out + j;
        for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
            uint64_t lo = 0, hi = 0;
            uint32_t peak = 0;
            if (c < ch)
                for (uint32_t i = 0; i < np; i++) {
                    const uint32_t *r = r0 + (uint64_t)i * REC + 4 * c;
                    const uint64_t x = (uint64_t)r[0] | (uint64_t)r[1] << 32;
                    lo += x;
                    hi += (uint64_t)r[2] + (lo < x ? 1u : 0u);
                    peak = r[3] > peak ? r[3] : peak;
                }
            o->sq_lo[c] = lo;
            o->sq_hi[c] = hi;
            o->peak[c] = peak;
        }
        o->frames = frames;
        o->reserved = 0;
    }
}

} // namespace nrg
