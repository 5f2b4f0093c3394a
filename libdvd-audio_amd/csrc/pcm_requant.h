// pcm_requant.h -- word-length reduction of decoded PCM, on the device: int32 PCM in either int32 layout -> int32 PCM in
// either int32 layout or the WAV payload, every value shifted down by s = bits_in - bits_out bits (truncated, rounded or
// dithered), clamped to the output range, and per channel the count of the values the clamp changed
// (include/dvda_mlp_hip.h states the contract).  The fifth client of pcm_tiles.h and the first pass that writes PCM.
// All of it is exact integer arithmetic.
//
//   value  q = (v + add) >> s as if in 64 bits, add = 0 / 2^(s-1) / 2^(s-1) + u1 - u2; clamp.  Computed in 32 bits as
//          (v >> s) + (((v & (2^s - 1)) + add) >> s), which is the same number and cannot overflow.  One __host__
//          __device__ function (value) that the kernel and dvda_pcm_hip_requant_value compile from the same text.
//   noise  u1, u2: two s-bit fields of a 64-bit word that is a function of (seed, absolute frame >> 2, channel) --
//          output number 8 Q + c + 1 of splitmix64 seeded with `seed` -- 16 bits of it per frame of the quad.  A lane
//          holds four consecutive frames of every channel, so where the stream's first absolute frame is a multiple of
//          4 it hashes once per channel; at any other phase twice.
//   tiles  the level report's: TILE frames aligned to the stream's START.  A workgroup takes a tile in chunks of CHUNK
//          = 4 * THREADS frames, lane t the frames 4 t .. 4 t + 3 of the chunk.
//   in     planar: one 16-byte load per channel where the plane's address allows it, else the four values one by one;
//          frame-major: the chunk's dwords into LDS, consecutive lanes consecutive 16-byte groups (dwords where the
//          address is not aligned), then each lane reads its own.  Only values inside the stream's `frames` are read.
//   out    planar: one 16-byte store per channel, or the four values; frame-major and the WAV payloads: the chunk's
//          values into LDS in output order (int32, 16-bit or 3 bytes each) and out as consecutive dwords, 16 bytes per
//          lane where the address allows it; the payload's last 1..3 bytes as bytes.  Nothing outside the stream's
//          output region is written.
//   place  every element is read and written by the same workgroup, all of a chunk's reads before its first write
//          (planar to planar: by the same thread), so input and output may be the same buffer with the same layout and
//          descriptors.
//   count  a thread counts per channel the values it clamped; per tile they are folded (pcmt::block_fold, four
//          channels in one word: a tile has at most 4096 of them) into TILE_WORDS words that the join sums per stream.
//          Every word a join reads was stored by this launch; no atomics.
//
// tests/requant_model.py restates the arithmetic with Python integers and in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_levels.h"
#include "pcm_tiles.h"

namespace rq {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;

constexpr uint32_t TILE = lvl::TILE;
constexpr uint32_t TILE_BLOCKS = 2048;      // workgroups of k_rq_tiles at most: they stride over the tile list
constexpr uint32_t REC = MAX_CHANNELS;      // words of a tile's record: the clamped values per channel
constexpr uint32_t CHUNK = 4 * THREADS;     // frames a workgroup holds at a time
static_assert(TILE % CHUNK == 0 && TILE < (1u << 16), "a tile is whole chunks, its counts fit 16 bits");

// what the kernels get of dvda_pcm_requant, judged by params_ok
struct Par {
    uint32_t s, mode, bits_out, pad;
    uint64_t seed;
};

__host__ __device__ __forceinline__ bool depth_ok(uint32_t b) { return b == 16 || b == 20 || b == 24; }

__host__ __device__ __forceinline__ bool params_ok(const dvda_pcm_requant &p)
{
    return depth_ok(p.bits_in) && depth_ok(p.bits_out) && p.bits_out <= p.bits_in && p.mode <= DVDA_RQ_TPDF &&
           p.reserved == 0;
}

__host__ __device__ __forceinline__ Par par_of(const dvda_pcm_requant &p)
{
    return Par{p.bits_in - p.bits_out, p.mode, p.bits_out, 0u, p.seed};
}

// the noise word of quad Q (= absolute frame >> 2) of channel c
__host__ __device__ __forceinline__ uint64_t noise_word(uint64_t seed, uint64_t Q, uint32_t c)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (8u * Q + c + 1u);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the 16 bits of frame F in its quad's word
__host__ __device__ __forceinline__ uint32_t noise_field(uint64_t word, uint32_t j) { return (uint32_t)(word >> (16u * j)) & 0xFFFFu; }

// THE value: v -> the clamped output value; *clipped += 1 when the clamp changed it.  field: noise_field (TPDF only).
__host__ __device__ __forceinline__ int32_t value(int32_t v, const Par &p, uint32_t field, uint32_t *clipped)
{
    int32_t q = v;
    if (p.s) {
        const uint32_t m = (1u << p.s) - 1u;
        int32_t add = 0;
        if (p.mode != DVDA_RQ_TRUNCATE)
            add = 1 << (p.s - 1);
        if (p.mode == DVDA_RQ_TPDF)
            add += (int32_t)(field & m) - (int32_t)((field >> 8) & m);
        // v = (v >> s) * 2^s + (v & m), so floor((v + add) / 2^s) = (v >> s) + floor(((v & m) + add) / 2^s): |v >> s| is
        // at most 2^27 and the second term lies in -1 .. 2
        q = (v >> p.s) + (((int32_t)((uint32_t)v & m) + add) >> p.s);
    }
    const int32_t hi = (int32_t)((1u << (p.bits_out - 1)) - 1u), lo = -hi - 1;
    const int32_t r = q < lo ? lo : q > hi ? hi : q;
    *clipped += r != q ? 1u : 0u;
    return r;
}

// frames of a stream the pass takes: the input descriptor must be one the reports take, the output descriptor must
// say the same frames and channels and have room for them
__host__ __device__ __forceinline__ uint64_t stream_frames(const dvda_pcm_crc_desc &in, const dvda_pcm_crc_desc &out)
{
    if (PCMT_NOT_TAKEN(in) || out.frames != in.frames || out.channels != in.channels || out.stride < out.frames)
        return 0;
    return in.frames;
}

// ---- step 1: tiles per stream
__global__ void k_rq_plan(const dvda_pcm_crc_desc *__restrict__ desc_in, const dvda_pcm_crc_desc *__restrict__ desc_out,
                          uint32_t n, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = lvl::tiles_of(stream_frames(desc_in[i], desc_out[i]));
}

constexpr uint32_t OUT_PLANAR = DVDA_PCM_PLANAR, OUT_FRAME_MAJOR = DVDA_PCM_INTERLEAVED, OUT_WAV24 = DVDA_PCM_WAV24,
                   OUT_WAV16 = DVDA_PCM_WAV16;

// n dwords between LDS and global memory, consecutive lanes consecutive 16-byte groups where `g` is 16-byte aligned
// (at most CHUNK * MAX_CHANNELS dwords: 8 groups per thread, all loads issued before the first store)
template <bool TO_LDS>
__device__ __forceinline__ void copy_dwords(uint32_t *s, uint32_t *g, uint32_t n, uint32_t t)
{
    uint32_t done = 0;
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
        const uint32_t n4 = n >> 2;
        uint4 *s4 = reinterpret_cast<uint4 *>(s), *g4 = reinterpret_cast<uint4 *>(g);
        uint4 q[MAX_CHANNELS];
#pragma unroll
        for (int i = 0; i < (int)MAX_CHANNELS; i++) {
            q[i] = make_uint4(0u, 0u, 0u, 0u);
            if (t + i * THREADS < n4)
                q[i] = TO_LDS ? g4[t + i * THREADS] : s4[t + i * THREADS];
        }
#pragma unroll
        for (int i = 0; i < (int)MAX_CHANNELS; i++)
            if (t + i * THREADS < n4) {
                if (TO_LDS)
                    s4[t + i * THREADS] = q[i];
                else
                    g4[t + i * THREADS] = q[i];
            }
        done = 4 * n4;
    }
    for (uint32_t d = done + t; d < n; d += THREADS) {
        if (TO_LDS)
            s[d] = g[d];
        else
            g[d] = s[d];
    }
}

// ---- step 3: every tile requantized, and its record.  The workgroups stride over the flat tile list (as many of it as
//      the caller's bound holds: rec has max_tiles records).  pcm and out may be the same buffer: no __restrict__.
template <bool IN_PLANAR, uint32_t OUT>
__global__ __launch_bounds__(THREADS, 4) void k_rq_tiles(const int32_t *pcm, const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                      int32_t *out, const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                      const uint64_t *__restrict__ frame0, uint32_t n, Par par,
                                                      const uint32_t *__restrict__ base, uint32_t *__restrict__ rec,
                                                      uint32_t max_tiles)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_buf[CHUNK * MAX_CHANNELS];
    __shared__ uint64_t s_red[WAVES];
    const uint32_t t = threadIdx.x, l = 4u * t;
    const bool tpdf = par.mode == DVDA_RQ_TPDF && par.s != 0;
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc di = desc_in[s], dn = desc_out[s];
        const uint64_t frames = stream_frames(di, dn);
        const uint32_t ti = b - base[s];
        if (ti >= lvl::tiles_of(frames))    // (counts that wrapped the scan: no tile of this stream, nothing is touched)
            continue;
        const uint32_t ch = di.channels;
        const uint64_t f0 = (uint64_t)ti * TILE;
        const uint32_t nf = frames - f0 < TILE ? (uint32_t)(frames - f0) : TILE;
        const uint64_t F0 = (frame0 ? frame0[s] : 0ull) + f0;
        const uint32_t phase = (uint32_t)F0 & 3u;       // of every lane's first frame: chunks and lanes are whole quads
        const int32_t *in_s = pcm + di.off;
        int32_t *out_s = out + dn.off;
        // a plane's quads are 16-byte groups in memory
        const bool in_16 = (reinterpret_cast<uintptr_t>(in_s) & 15u) == 0 && (ch == 1 || (di.stride & 3u) == 0);
        const bool out_16 = (reinterpret_cast<uintptr_t>(out_s) & 15u) == 0 && (ch == 1 || (dn.stride & 3u) == 0);
        uint32_t cnt[MAX_CHANNELS] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t k0 = 0; k0 < nf; k0 += CHUNK) {
            const uint32_t nfc = nf - k0 < CHUNK ? nf - k0 : CHUNK;     // frames of the chunk
            const uint64_t fc = f0 + k0;                                // the chunk's first frame in the stream
            const bool whole = l + 4u <= nfc;                           // the lane's quad lies inside the stream
            int32_t v[MAX_CHANNELS][4];
            if (IN_PLANAR) {
#pragma unroll
                for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                    if (c < ch) {
                        const int32_t *p = in_s + (uint64_t)c * di.stride + fc + l;
                        if (in_16 && whole) {
                            const int4 q = *reinterpret_cast<const int4 *>(p);
                            v[c][0] = q.x, v[c][1] = q.y, v[c][2] = q.z, v[c][3] = q.w;
                        } else {
#pragma unroll
                            for (uint32_t j = 0; j < 4; j++)
                                v[c][j] = l + j < nfc ? p[j] : 0;
                        }
                    }
            } else {
                copy_dwords<true>(s_buf, const_cast<uint32_t *>(reinterpret_cast<const uint32_t *>(in_s + fc * ch)), nfc * ch, t);
                __syncthreads();
                // (a lane whose quad lies inside the chunk -- all of them but in a stream's last chunk -- asks nothing per value)
                auto take = [&](auto all) {
#pragma unroll
                    for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                        if (c < ch) {
#pragma unroll
                            for (uint32_t j = 0; j < 4; j++)
                                v[c][j] = all.value || l + j < nfc ? (int32_t)s_buf[l * ch + (j * ch + c)] : 0;
                        }
                };
                if (whole)
                    take(std::true_type());
                else
                    take(std::false_type());
                if (OUT != OUT_PLANAR)
                    __syncthreads();        // (s_buf is filled again below)
            }
            const uint64_t F = F0 + k0 + l;         // the lane's first absolute frame
#pragma unroll
            for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                if (c < ch) {
                    uint64_t z = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) {
                        const uint32_t jj = (phase + j) & 3u;
                        if (tpdf && (j == 0 || jj == 0))
                            z = noise_word(par.seed, (F + j) >> 2, c);
                        uint32_t cl = 0;
                        v[c][j] = value(v[c][j], par, noise_field(z, jj), &cl);
                        cnt[c] += cl;               // (a value outside the chunk stands as 0 here, which no mode clamps)
                    }
                }
            if (OUT == OUT_PLANAR) {
#pragma unroll
                for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                    if (c < ch) {
                        int32_t *o = out_s + (uint64_t)c * dn.stride + fc + l;
                        if (out_16 && whole) {
                            *reinterpret_cast<int4 *>(o) = make_int4(v[c][0], v[c][1], v[c][2], v[c][3]);
                        } else {
#pragma unroll
                            for (uint32_t j = 0; j < 4; j++)
                                if (l + j < nfc)
                                    o[j] = v[c][j];
                        }
                    }
                if (!IN_PLANAR)
                    __syncthreads();        // (s_buf has been read: the next chunk fills it)
            } else {
                // the chunk's values in output order; an in-range value's low bytes are write_signed of it
                const uint32_t nb = OUT == OUT_FRAME_MAJOR ? 4u : OUT == OUT_WAV24 ? 3u : 2u;
                auto put = [&](auto all) {
#pragma unroll
                    for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                        if (c < ch) {
#pragma unroll
                            for (uint32_t j = 0; j < 4; j++)
                                if (all.value || l + j < nfc) {
                                    const uint32_t i = l * ch + (j * ch + c), x = (uint32_t)v[c][j];
                                    if (OUT == OUT_FRAME_MAJOR) {
                                        s_buf[i] = x;
                                    } else if (OUT == OUT_WAV16) {
                                        reinterpret_cast<uint16_t *>(s_buf)[i] = (uint16_t)x;
                                    } else {
                                        uint8_t *o = reinterpret_cast<uint8_t *>(s_buf) + 3u * i;
                                        o[0] = (uint8_t)x, o[1] = (uint8_t)(x >> 8), o[2] = (uint8_t)(x >> 16);
                                    }
                                }
                        }
                };
                if (whole)
                    put(std::true_type());
                else
                    put(std::false_type());
                __syncthreads();
                // (a chunk in front of the last one is CHUNK frames: its bytes are whole dwords, so every chunk starts on one)
                const uint32_t bytes = nfc * ch * nb;
                uint8_t *o = reinterpret_cast<uint8_t *>(out_s) + fc * ch * nb;
                copy_dwords<false>(s_buf, reinterpret_cast<uint32_t *>(o), bytes >> 2, t);
                if (t < (bytes & 3u))
                    o[(bytes & ~3u) + t] = reinterpret_cast<const uint8_t *>(s_buf)[(bytes & ~3u) + t];
                __syncthreads();            // (s_buf has been read: the next chunk fills it)
            }
        }
        // four channels' counts in one word: 16 bits each, at most TILE per tile
        uint64_t lo = (uint64_t)cnt[0] | (uint64_t)cnt[1] << 16 | (uint64_t)cnt[2] << 32 | (uint64_t)cnt[3] << 48;
        uint64_t hi = (uint64_t)cnt[4] | (uint64_t)cnt[5] << 16 | (uint64_t)cnt[6] << 32 | (uint64_t)cnt[7] << 48;
        lo = pcmt::block_fold(lo, s_red, pcmt::FoldSum());
        hi = pcmt::block_fold(hi, s_red, pcmt::FoldSum());
        if (t == 0) {
            uint32_t *o = rec + (uint64_t)b * REC;
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) {
                o[c] = (uint32_t)(lo >> (16u * c)) & 0xFFFFu;
                o[4 + c] = (uint32_t)(hi >> (16u * c)) & 0xFFFFu;
            }
        }
    }
}

// ---- step 4: one workgroup per stream sums the stream's records.  A stream whose tiles do not all lie inside the
//      caller's bound is reported as zeros.
__global__ __launch_bounds__(THREADS) void k_rq_join(const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                     const dvda_pcm_crc_desc *__restrict__ desc_out, uint32_t n,
                                                     const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                     uint32_t max_tiles, dvda_pcm_requant_report *__restrict__ out)
{
    __shared__ uint64_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    uint64_t frames = stream_frames(desc_in[s], desc_out[s]);
    const uint32_t first = base[s], n_t = lvl::tiles_of(frames);
    if ((uint64_t)first + n_t > max_tiles)
        frames = 0;
    const uint32_t ch = frames ? desc_in[s].channels : 0u, turns = frames ? n_t : 0u;
    const uint32_t *r0 = rec + (uint64_t)first * REC;
    if (threadIdx.x == 0)
        out[s].frames = frames;
    for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
        uint64_t sum = 0;
        if (c < ch)
            for (uint32_t i = threadIdx.x; i < turns; i += THREADS)
                sum += r0[(uint64_t)i * REC + c];
        sum = pcmt::block_fold(sum, s_red, pcmt::FoldSum());
        if (threadIdx.x == 0)
            out[s].clipped[c] = sum;
    }
}

} // namespace rq
