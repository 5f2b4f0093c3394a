// pcm_digest.h -- CRC-32 of the WAV payload of decoded PCM, on the device, from whichever layout the decode wrote
// (include/dvda_mlp_hip.h states the contract: zlib.crc32 of the data chunk dvda2wav writes).
//
// CRC as field arithmetic, as mlp_check.h does for CRC-8: GF(2)[x] / P in the reflected representation -- bit 31 of a
// word is x^0, "times x" is a right shift with a conditional XOR of 0xEDB88320.  Raw CRC = initial value 0, no final
// XOR; it is linear, leading zero bytes do not change it, and one little-endian payload dword d advances a state s to
// (s ^ d) * x^32.  So raw(D) = sum d_j * x^(32 (N - j)) over the N dwords, and
//     zlib(D) = raw(D) ^ 0xFFFFFFFF * x^(8 n) ^ 0xFFFFFFFF.
//
//   tiles  a payload is cut into tiles of TILE bytes ALIGNED TO ITS END: the first tile of a stream is the ragged one,
//          bytes in front of the payload read as zero -- every tile has the same length and the same weights
//   lanes  a tile is WAVES regions of 64 * K dwords; lane l of a wave takes the region's dwords l, l + 64, ... (coalesced
//          loads) by Horner's rule acc = acc * x^2048 ^ d, the constant multiply through four 256-entry tables in LDS;
//          then acc is weighed with x^(32 + 32 (63 - l)) * x^(2048 K (WAVES - 1 - wave)) and everything XOR-reduced
//   join   one workgroup per stream folds the stream's tile values, counted from the end, thread j taking tiles
//          j, j + JOIN, ... by Horner with x^(8 TILE JOIN), weighs with x^(8 TILE j), XOR-reduces, and adds the one
//          variable power, x^(8 n) for the initial value, by square-and-multiply
//
// A payload dword is whatever the layout makes of it: one Src per layout (WAV payload: two aligned loads and a byte
// funnel; int32 frame-major / planar: the two neighbouring values it touches, through write_signed), one kernel body.
// tests/digest_model.py restates all of it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_tiles.h"

namespace crc {

using pcmt::find_stream;
using pcmt::THREADS;
using pcmt::WAVES;

constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t ONE = 0x80000000u;       // x^0
constexpr int K = 16;                       // dwords per lane and tile
constexpr uint32_t TILE = DVDA_CRC_TILE_BYTES;
constexpr uint32_t JOIN = DVDA_CRC_JOIN_TILES;
static_assert(TILE == (uint32_t)THREADS * K * 4 && TILE % 256 == 0, "a tile is K dwords per lane of one workgroup");
static_assert(JOIN == (uint32_t)THREADS, "the join folds one tile per thread and turn");
constexpr uint32_t TILE_BLOCKS = 4096;      // workgroups of k_crc_tiles at most: they stride over the tile list

__host__ __device__ constexpr uint32_t mulx(uint32_t a) { return (a >> 1) ^ ((a & 1u) ? POLY : 0u); }

__host__ __device__ constexpr uint32_t gfmul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) {
        r ^= (b & (ONE >> i)) ? a : 0u;
        a = mulx(a);
    }
    return r;
}

// x^e by square-and-multiply (the one variable power of a digest)
__host__ __device__ constexpr uint32_t xpow(uint64_t e)
{
    uint32_t r = ONE, p = ONE >> 1;
    while (e) {
        if (e & 1u)
            r = gfmul(r, p);
        p = gfmul(p, p);
        e >>= 1;
    }
    return r;
}

struct Tables {
    uint32_t mul[4 * 256];      // v * x^2048 = mul[v & 255] ^ mul[256 + (v >> 8 & 255)] ^ mul[512 + (v >> 16 & 255)] ^ mul[768 + (v >> 24)]
    uint32_t lane_w[THREADS];   // thread (wave, lane): x^(32 (64 K (WAVES - 1 - wave) + 64 - lane))
    uint32_t join_w[JOIN];      // thread j of the join: x^(8 TILE j)
    uint32_t join_step;         // x^(8 TILE JOIN)
};

constexpr Tables make_tables()
{
    Tables t{};
    const uint32_t c = xpow(2048);
    for (int k = 0; k < 4; k++)
        for (uint32_t b = 0; b < 256; b++)
            t.mul[k * 256 + b] = gfmul(b << (8 * k), c);
    uint32_t w = ONE;
    for (int i = THREADS - 1; i >= 0; i--) {        // thread i's dword is 32 bits further from the end than thread i + 1's
        for (int s = 0; s < 32; s++)
            w = mulx(w);
        t.lane_w[i] = w;
        if ((i & 63) == 0)                           // the wave in front: its last lane-dword sits 64 (K - 1) dwords further
            w = gfmul(w, xpow(2048ull * (K - 1)));
    }
    const uint32_t tile = xpow(8ull * TILE);
    w = ONE;
    for (uint32_t j = 0; j < JOIN; j++) {
        t.join_w[j] = w;
        w = gfmul(w, tile);
    }
    t.join_step = w;
    return t;
}

__device__ const Tables d_tab = make_tables();

// payload bytes of a stream (0 for a descriptor outside what the kernels take)
__host__ __device__ __forceinline__ uint64_t stream_bytes(const dvda_pcm_crc_desc &d, uint32_t nb)
{
    if (PCMT_NOT_TAKEN(d))
        return 0;
    return d.frames * d.channels * nb;
}

__host__ __device__ __forceinline__ uint32_t tiles_of(uint64_t bytes) { return (uint32_t)((bytes + TILE - 1) / TILE); }

// ---- step 1: tiles per stream (the index's exclusive scan runs over them)
__global__ void k_crc_plan(const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t nb, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = tiles_of(stream_bytes(desc[i], nb));
}

__host__ __device__ __forceinline__ uint32_t write_signed(int32_t v, uint32_t low, uint32_t sign)
{
    return ((uint32_t)v & low) | (v < 0 ? sign : 0u);
}

// ---- payload dwords, per layout (host-callable too: a CPU program can walk a tile the way a workgroup does).
//      setup(): once per tile, p = payload position of the tile's first byte (negative
//      inside the zero prefix of a stream's first tile); dword(g): payload bytes p + 4 g .. p + 4 g + 3.
constexpr int SRC_WAV = 0, SRC_FRAME_MAJOR = 1, SRC_PLANAR = 2;

// DVDA_PCM_WAV24 / WAV16: the payload lies there, starting dword-aligned; a tile's dwords are misaligned against
// memory by the stream's length mod 4, the same for every tile of the stream
struct SrcWav {
    const uint32_t *words;
    int64_t first;      // index of the aligned word holding the tile's first byte
    int64_t limit;      // words that hold payload: nothing at or behind it is read, whatever the tile's position says
    uint32_t sh;        // 8 * misalignment

    __host__ __device__ __forceinline__ void setup(const int32_t *pcm, const dvda_pcm_crc_desc &d, uint64_t bytes, uint32_t, int64_t p)
    {
        words = reinterpret_cast<const uint32_t *>(pcm) + d.off;
        sh = 8u * (uint32_t)(bytes & 3u);
        limit = (int64_t)((bytes + 3u) >> 2);
        first = (p - (int64_t)(bytes & 3u)) >> 2;       // (p = bytes mod 4, mod 4: exact)
    }
    __host__ __device__ __forceinline__ uint32_t dword(uint32_t g) const
    {
        const int64_t i = first + g;
        const uint32_t lo = (i >= 0 && i < limit) ? words[i] : 0u;
        // (aligned stream: the word behind the last one is not the stream's, and not read)
        const uint32_t hi = (sh && i + 1 >= 0 && i + 1 < limit) ? words[i + 1] : 0u;
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
    }
};

// int32 layouts: a dword is assembled from the two values it touches (24 bits: at any of three byte positions; 16 bits:
// a tile starts on a value, payload and TILE both being even, so a dword is exactly two values).
// PLANAR: value (frame, channel) at channel * stride + frame; frame-major: at frame * channels + channel.
template <bool PLANAR>
struct SrcInt {
    static constexpr uint32_t BIAS = 3 * TILE;      // multiple of 2 and 3, more than a zero prefix is long
    const int32_t *base;
    uint64_t stride, total;     // values of the stream
    uint64_t q0, f0;            // first value of the tile that exists (0 in a stream's first tile), and its frame
    uint32_t c0, skip;          // its channel; values of the zero prefix in front of it
    uint32_t b0, nb, ch, magic, low, sign;

    __host__ __device__ __forceinline__ void setup(const int32_t *pcm, const dvda_pcm_crc_desc &d, uint64_t, uint32_t nb_, int64_t p)
    {
        base = pcm + d.off;
        stride = d.stride;
        ch = d.channels;
        nb = nb_;
        total = d.frames * ch;
        low = (1u << (8 * nb - 1)) - 1u;
        sign = 1u << (8 * nb - 1);
        magic = 0xFFFFFFFFu / ch + 1u;              // y / ch = umulhi(y, magic) for y < 2^17, ch in 2..8
        const uint64_t pb = (uint64_t)(p + (int64_t)BIAS);
        const uint64_t qb = nb == 3 ? pb / 3u : pb >> 1;
        b0 = (uint32_t)(pb - qb * nb);
        const int64_t qs = (int64_t)qb - (int64_t)(BIAS / nb);
        skip = qs < 0 ? (uint32_t)(-qs) : 0u;
        q0 = qs < 0 ? 0ull : (uint64_t)qs;
        if (PLANAR) {
            f0 = q0 / ch;
            c0 = (uint32_t)(q0 - f0 * ch);
        }
    }
    __host__ __device__ __forceinline__ uint32_t value(int32_t rel) const
    {
        if (rel < 0 || q0 + (uint32_t)rel >= total)
            return 0u;
        uint64_t at;
        if (PLANAR) {
            const uint32_t y = c0 + (uint32_t)rel;
            const uint32_t fr = ch == 1 ? y : (uint32_t)(((uint64_t)y * magic) >> 32);
            at = (uint64_t)(y - fr * ch) * stride + f0 + fr;
        } else {
            at = q0 + (uint32_t)rel;
        }
        return write_signed(base[at], low, sign);
    }
    __host__ __device__ __forceinline__ uint32_t dword(uint32_t g) const
    {
        const uint32_t x = 4u * g + b0;
        const uint32_t dq = nb == 3 ? x / 3u : x >> 1;
        const uint32_t b = x - dq * nb;
        const int32_t rel = (int32_t)dq - (int32_t)skip;
        const uint64_t w = value(rel) | ((uint64_t)value(rel + 1) << (8 * nb));
        return (uint32_t)(w >> (8 * b));
    }
};

__host__ __device__ __forceinline__ uint32_t mul_x2048(const uint32_t *s_mul, uint32_t v)
{
    return s_mul[v & 255u] ^ s_mul[256u + ((v >> 8) & 255u)] ^ s_mul[512u + ((v >> 16) & 255u)] ^ s_mul[768u + (v >> 24)];
}

// ---- step 3: the raw CRC of every tile.  The workgroups stride over the flat tile list (as many of it as the
//      caller's bound holds: tile_val has max_tiles entries).
template <int LAYOUT>
__global__ __launch_bounds__(THREADS) void k_crc_tiles(const int32_t *__restrict__ pcm,
                                                       const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t nb,
                                                       const uint32_t *__restrict__ base, uint32_t *__restrict__ tile_val,
                                                       uint32_t max_tiles)
{
    __shared__ uint32_t s_mul[4 * 256];
    __shared__ uint32_t s_red[WAVES];
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += THREADS)
        s_mul[i] = d_tab.mul[i];
    const uint32_t weight = d_tab.lane_w[threadIdx.x];
    __syncthreads();
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    const uint32_t g0 = (threadIdx.x >> 6) * (64u * K) + (threadIdx.x & 63u);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = find_stream(base, n, b);
        const dvda_pcm_crc_desc d = desc[s];
        const uint64_t bytes = stream_bytes(d, nb);
        const uint32_t left = tiles_of(bytes) - (b - base[s]);      // tiles from this one to the stream's end
        const int64_t p = (int64_t)bytes - (int64_t)left * TILE;
        typename std::conditional<LAYOUT == SRC_WAV, SrcWav, SrcInt<LAYOUT == SRC_PLANAR>>::type src;
        src.setup(pcm, d, bytes, nb, p);
        uint32_t v[K];
#pragma unroll
        for (int i = 0; i < K; i++)
            v[i] = src.dword(g0 + 64u * i);
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < K; i++)
            acc = mul_x2048(s_mul, acc) ^ v[i];
        const uint32_t r = pcmt::block_fold(gfmul(acc, weight), s_red, pcmt::FoldXor());
        if (threadIdx.x == 0)
            tile_val[b] = r;
    }
}

// ---- step 4: one workgroup per stream joins the stream's tile values and finishes the digest.  A stream whose tiles
//      do not all lie inside the caller's bound is reported as (0, 0).
__global__ __launch_bounds__(THREADS) void k_crc_join(const dvda_pcm_crc_desc *__restrict__ desc, uint32_t n, uint32_t nb,
                                                      const uint32_t *__restrict__ base,
                                                      const uint32_t *__restrict__ tile_val, uint32_t max_tiles,
                                                      uint32_t *__restrict__ crc_out, uint64_t *__restrict__ nbytes_out)
{
    __shared__ uint32_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    uint64_t bytes = stream_bytes(desc[s], nb);
    const uint32_t first = base[s], n_t = tiles_of(bytes);
    if ((uint64_t)first + n_t > max_tiles)
        bytes = 0;
    uint32_t acc = 0;
    if (bytes && threadIdx.x < n_t) {
        // r counts tiles from the stream's end; this thread's furthest one first
        const uint32_t step = d_tab.join_step;
        for (int64_t r = threadIdx.x + (uint64_t)((n_t - 1 - threadIdx.x) / JOIN) * JOIN; r >= 0; r -= JOIN)
            acc = gfmul(acc, step) ^ tile_val[first + (n_t - 1 - (uint32_t)r)];
        acc = gfmul(acc, d_tab.join_w[threadIdx.x]);
    }
    const uint32_t raw = pcmt::block_fold(acc, s_red, pcmt::FoldXor());
    if (threadIdx.x == 0) {
        crc_out[s] = bytes ? raw ^ gfmul(0xFFFFFFFFu, xpow(8ull * bytes)) ^ 0xFFFFFFFFu : 0u;
        nbytes_out[s] = bytes;
    }
}

} // namespace crc
