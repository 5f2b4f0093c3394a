// pcm_mix.h -- the channel mix of decoded PCM, on the device: int32 PCM of `in` channels in either int32 layout -> int32
// PCM of `out` channels in either int32 layout, every output value a row of Q30 coefficients over the frame's input
// values (64-bit accumulation; one rounding; clamped to `bits`), and per OUTPUT channel the count of the values the clamp
// changed (include/dvda_mlp_hip.h states the contract).  The eighth client of pcm_tiles.h and the first pass whose output
// has another channel count than its input.  All of it is exact integer arithmetic.
//
//   value  acc = sum_c coef[o][c] x[c] in int64 (a valid row has sum |coef| <= 2^31: no int32 input overflows it), y =
//          clamp((acc + 2^29) >> 30).  One text for the kernel and the host: mad() and finish(); value() is the two over
//          one frame and dvda_pcm_hip_mix_value compiles it.  (Both are pcm_write.h's.)
//   take   THE predicate of plan, tiles and join: the matrix valid, its channel counts those of the two descriptors, the
//          output descriptor exactly the input's frames with room for them.  The matrices are device arrays, so it is
//          the kernels that judge them.
//   tiles  the requantizer's: TILE frames aligned to the stream's START.  A workgroup takes a tile in chunks of CHUNK =
//          4 * THREADS frames and holds a chunk in LDS as planes: value (c, f) at s_buf[c * PITCH + f].
//   in     the chunk's dwords in memory order, 16 bytes per lane: a plane (planar) or the whole run of frames
//          (frame-major) is cut at the 16-byte boundaries of its ADDRESS, so the wide loads serve any 4-byte alignment of
//          `off` and any parity of a stride; the 0..3 dwords in front of the first boundary and behind the last one go
//          one by one.  A frame-major dword d of the run is value (d mod ch, d div ch): scattered into its plane.  No
//          lane walks global memory at a stride of `channels` dwords.  Only values inside the stream's `frames` are read.
//   mix    lane t takes the frames t, t + THREADS, ... of the chunk: consecutive lanes read and write consecutive words
//          of a plane, so no two lanes of a wave meet on a bank.  A lane reads its frames' column, then writes the
//          outputs into the same column of the planes 0 .. out - 1 -- the planes are reused and no other lane has
//          business in that column, so there is no barrier between the two.  PITCH = CHUNK + 4: the scatter's lanes,
//          which differ in plane and frame at once, spread over the banks (4 PITCH = 16 mod 32).
//   coef   a tile belongs to one stream: the matrix is wave-uniform.  A row is one scalar load of 32 bytes where it is
//          used (the whole matrix held in 64 SGPRs across the chunk loop was spilled through v_writelane), zeroed
//          outside [in), and is the SGPR operand of the multiply-add, which is written out (mad); a zero coefficient is
//          skipped by a wave-uniform branch that covers the lane's four frames.
//   out    mirrors the input side: planes out as they lie, frame-major gathered from the planes into 16-byte groups.
//          Nothing outside the stream's output region is written.
//   count  the clamped values per OUTPUT channel, a record of REC words per tile, summed by the join (pcm_write.h).
//
// tests/mix_model.py restates the arithmetic with Python integers and in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvda_mlp_hip.h"
#include "pcm_levels.h"
#include "pcm_tiles.h"
#include "pcm_write.h"

namespace mix {

using pcmt::MAX_CHANNELS;
using pcmt::THREADS;
using pcmt::WAVES;
using pcmw::depth_ok;
using pcmw::div_small;
using pcmw::finish;
using pcmw::mad;
using pcmw::REC;

constexpr uint32_t TILE = lvl::TILE;
constexpr uint32_t TILE_BLOCKS = 2048;      // workgroups of k_mix_tiles at most: they stride over the tile list
constexpr uint32_t PER_LANE = 4;            // frames of a chunk a lane mixes
constexpr uint32_t CHUNK = PER_LANE * THREADS;      // frames a workgroup holds at a time
constexpr uint32_t PITCH = CHUNK + 4;       // words between the planes of a chunk in LDS
constexpr uint32_t BATCH = 4;               // 16-byte loads a lane has in flight on the input side
static_assert(TILE % CHUNK == 0 && TILE < (1u << 16), "a tile is whole chunks, its counts fit 16 bits");
static_assert(CHUNK / 4 <= THREADS, "a plane of a chunk is at most one 16-byte group per lane");

// the channel counts in range and every used row's sum of |coef| at most 2^31
__host__ __device__ __forceinline__ bool valid(const dvda_pcm_mix &m)
{
    if (m.in_channels == 0 || m.in_channels > MAX_CHANNELS || m.out_channels == 0 || m.out_channels > MAX_CHANNELS)
        return false;
    bool ok = true;
    for (uint32_t o = 0; o < MAX_CHANNELS; o++) {
        uint64_t sum = 0;
        for (uint32_t c = 0; c < MAX_CHANNELS; c++) {
            const int64_t g = m.coef[o][c];
            sum += c < m.in_channels ? (uint64_t)(g < 0 ? -g : g) : 0ull;
        }
        ok = ok && (o >= m.out_channels || sum <= (1ull << 31));
    }
    return ok;
}

// THE value: output channel o of the frame whose in_channels values are x[].  (In the kernel the coefficient of
// pcmw::mad is wave-uniform: from `acc += (int64_t)g * x` with such a g the compiler extends g to 64 bits on the scalar
// side and multiplies in pieces -- v_mad_u64_u32, v_mul_lo_u32, adds.)
__host__ __device__ __forceinline__ int32_t value(const int32_t *x, const dvda_pcm_mix &m, uint32_t o, uint32_t bits,
                                                  uint32_t *clipped)
{
    int64_t acc = 0;
    for (uint32_t c = 0; c < m.in_channels; c++)
        mad(acc, m.coef[o][c], x[c]);
    return finish(acc, bits, clipped);
}

// frames of a stream the pass takes (0: the stream is not taken, or has none): the input descriptor must be one the
// reports take, the matrix valid with the channel counts of the two descriptors, and the output descriptor must say the
// same frames and have room for them
__host__ __device__ __forceinline__ uint64_t take(const dvda_pcm_crc_desc &in, const dvda_pcm_crc_desc &out,
                                                  const dvda_pcm_mix &m)
{
    if (PCMT_NOT_TAKEN(in) || !valid(m) || m.in_channels != in.channels || m.out_channels != out.channels ||
        out.frames != in.frames || out.stride < out.frames)
        return 0;
    return in.frames;
}

// ---- step 1: tiles per stream
__global__ void k_mix_plan(const dvda_pcm_crc_desc *__restrict__ desc_in, const dvda_pcm_crc_desc *__restrict__ desc_out,
                           const dvda_pcm_mix *__restrict__ mat, uint32_t n, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        cnt[i] = lvl::tiles_of(take(desc_in[i], desc_out[i], mat[i]));
}

// dwords of a run at `p` in front of its first 16-byte boundary (all n where it does not reach one)
__device__ __forceinline__ uint32_t head_of(const void *p, uint32_t n)
{
    const uint32_t h = (uint32_t)(-(reinterpret_cast<uintptr_t>(p) >> 2)) & 3u;
    return h < n ? h : n;
}

// ---- n <= CHUNK words between a plane of the chunk in LDS (row) and its n values in global memory (g): the 16-byte
//      groups of g's address one per lane, the dwords on either side of them one by one
struct Row {
    uint32_t head, groups, tail0, tail;     // tail0: the first dword behind the groups
    __device__ __forceinline__ Row(const void *g, uint32_t n)
    {
        head = head_of(g, n);
        groups = (n - head) >> 2;
        tail0 = head + 4u * groups;
        tail = n - tail0;
    }
    // what lane t moves one by one: a dword of the head or of the tail (n: none)
    __device__ __forceinline__ uint32_t single(uint32_t t, uint32_t n) const
    {
        return t < head ? t : t - head < tail ? tail0 + (t - head) : n;
    }
};

// a row of the matrix as one value (the struct aligns it to 4 bytes only)
typedef int32_t Row8 __attribute__((ext_vector_type(8), aligned(4)));

// ---- step 3: every tile mixed, and its record.  The workgroups stride over the flat tile list (as many of it as the
//      caller's bound holds: rec has max_tiles records).
template <bool IN_PLANAR, bool OUT_PLANAR>
__global__ __launch_bounds__(THREADS, 4) void k_mix_tiles(const int32_t *__restrict__ pcm,
                                                       const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                       int32_t *__restrict__ out,
                                                       const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                       const dvda_pcm_mix *__restrict__ mat, uint32_t n, uint32_t bits,
                                                       const uint32_t *__restrict__ base, uint32_t *__restrict__ rec,
                                                       uint32_t max_tiles)
{
    __shared__ __attribute__((aligned(16))) int32_t s_buf[MAX_CHANNELS * PITCH];
    __shared__ uint64_t s_red[WAVES];
    const uint32_t t = threadIdx.x;
    const uint32_t total = pcmt::list_tiles(base, n, max_tiles);
    for (uint32_t b = blockIdx.x; b < total; b += gridDim.x) {
        const uint32_t s = pcmt::find_stream(base, n, b);
        const dvda_pcm_crc_desc di = desc_in[s], dn = desc_out[s];
        const dvda_pcm_mix &m = mat[s];
        const uint64_t frames = take(di, dn, m);
        const uint32_t ti = b - base[s];
        if (ti >= lvl::tiles_of(frames))    // (counts that wrapped the scan: no tile of this stream, nothing is touched)
            continue;
        const uint32_t ich = di.channels, och = dn.channels;
        const uint32_t inv_i = pcmw::inv_of(ich), inv_o = pcmw::inv_of(och);
        const uint64_t f0 = (uint64_t)ti * TILE;
        const uint32_t nf = frames - f0 < TILE ? (uint32_t)(frames - f0) : TILE;
        const int32_t *in_s = pcm + di.off;
        int32_t *out_s = out + dn.off;
        pcmw::ClipCount cnt;
        for (uint32_t k0 = 0; k0 < nf; k0 += CHUNK) {
            const uint32_t nfc = nf - k0 < CHUNK ? nf - k0 : CHUNK;     // frames of the chunk
            const uint64_t fc = f0 + k0;                                // the chunk's first frame in the stream
            // ---- in: the chunk as planes in s_buf
            if (IN_PLANAR || ich == 1) {
                // (BATCH planes at a time: their loads are all asked for before the first of them is stored)
#pragma unroll 1
                for (uint32_t c0 = 0; c0 < ich; c0 += BATCH) {
                    int4 q[BATCH];
                    int32_t one[BATCH];
#pragma unroll
                    for (uint32_t k = 0; k < BATCH; k++)
                        if (c0 + k < ich) {
                            const int32_t *p = in_s + (uint64_t)(c0 + k) * di.stride + fc;
                            const Row r(p, nfc);
                            const uint32_t i = r.single(t, nfc);
                            if (t < r.groups)
                                q[k] = *reinterpret_cast<const int4 *>(p + r.head + 4u * t);
                            if (i < nfc)
                                one[k] = p[i];
                        }
#pragma unroll
                    for (uint32_t k = 0; k < BATCH; k++)
                        if (c0 + k < ich) {
                            const Row r(in_s + (uint64_t)(c0 + k) * di.stride + fc, nfc);
                            const uint32_t i = r.single(t, nfc);
                            int32_t *row = s_buf + (c0 + k) * PITCH;
                            if (t < r.groups) {
                                if (r.head == 0) {
                                    *reinterpret_cast<int4 *>(row + 4u * t) = q[k];
                                } else {
                                    int32_t *w = row + r.head + 4u * t;
                                    w[0] = q[k].x, w[1] = q[k].y, w[2] = q[k].z, w[3] = q[k].w;
                                }
                            }
                            if (i < nfc)
                                row[i] = one[k];
                        }
                }
            } else {
                const int32_t *p = in_s + fc * ich;
                const uint32_t nd = nfc * ich;
                const Row r(p, nd);
                const uint32_t i = r.single(t, nd);
                int32_t one = 0;
                if (i < nd)
                    one = p[i];
#pragma unroll 1
                for (uint32_t g0 = t; g0 < r.groups; g0 += BATCH * THREADS) {
                    int4 q[BATCH];
#pragma unroll
                    for (uint32_t k = 0; k < BATCH; k++)
                        if (g0 + k * THREADS < r.groups)
                            q[k] = *reinterpret_cast<const int4 *>(p + r.head + 4u * (g0 + k * THREADS));
#pragma unroll
                    for (uint32_t k = 0; k < BATCH; k++)
                        if (g0 + k * THREADS < r.groups) {
                            const uint32_t d = r.head + 4u * (g0 + k * THREADS);
                            uint32_t f = div_small(d, ich, inv_i), c = d - f * ich;
                            const int32_t v[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
                            for (uint32_t j = 0; j < 4; j++) {
                                s_buf[c * PITCH + f] = v[j];
                                c++;
                                if (c == ich)
                                    c = 0, f++;
                            }
                        }
                }
                if (i < nd) {
                    const uint32_t f = div_small(i, ich, inv_i);
                    s_buf[(i - f * ich) * PITCH + f] = one;
                }
            }
            __syncthreads();
            // ---- mix: the lane's frames t + j * THREADS, in place in its own column of the planes
            {
                int32_t x[MAX_CHANNELS][PER_LANE];
#pragma unroll
                for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                    if (c < ich) {
#pragma unroll
                        for (uint32_t j = 0; j < PER_LANE; j++)
                            x[c][j] = s_buf[c * PITCH + t + j * THREADS];
                    }
#pragma unroll
                for (uint32_t o = 0; o < MAX_CHANNELS; o++)
                    if (o < och) {
                        // the row: wave-uniform, on the scalar side; zero where the contract ignores it
                        const Row8 gr = *reinterpret_cast<const Row8 *>(m.coef[o]);     // (one scalar load of 32 bytes)
                        int32_t g[MAX_CHANNELS];
#pragma unroll
                        for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                            g[c] = __builtin_amdgcn_readfirstlane(c < ich ? gr[c] : 0);
                        int64_t acc[PER_LANE];
#pragma unroll
                        for (uint32_t j = 0; j < PER_LANE; j++)
                            acc[j] = 0;
#pragma unroll
                        for (uint32_t c = 0; c < MAX_CHANNELS; c++)
                            if (g[c] != 0) {
#pragma unroll
                                for (uint32_t j = 0; j < PER_LANE; j++)
                                    mad(acc[j], g[c], x[c][j]);
                            }
                        uint32_t cl = 0;
#pragma unroll
                        for (uint32_t j = 0; j < PER_LANE; j++) {
                            uint32_t one = 0;
                            s_buf[o * PITCH + t + j * THREADS] = finish(acc[j], bits, &one);
                            cl += t + j * THREADS < nfc ? one : 0u;     // (behind the chunk's end: not a value)
                        }
                        cnt.add(o, cl);
                    }
            }
            __syncthreads();
            // ---- out: the planes 0 .. och - 1 as the output lies in memory
            if (OUT_PLANAR || och == 1) {
#pragma unroll
                for (uint32_t o = 0; o < MAX_CHANNELS; o++)
                    if (o < och) {
                        int32_t *p = out_s + (uint64_t)o * dn.stride + fc;
                        const Row r(p, nfc);
                        const uint32_t i = r.single(t, nfc);
                        const int32_t *row = s_buf + o * PITCH;
                        if (t < r.groups) {
                            int4 q;
                            if (r.head == 0) {
                                q = *reinterpret_cast<const int4 *>(row + 4u * t);
                            } else {
                                const int32_t *w = row + r.head + 4u * t;
                                q = make_int4(w[0], w[1], w[2], w[3]);
                            }
                            *reinterpret_cast<int4 *>(p + r.head + 4u * t) = q;
                        }
                        if (i < nfc)
                            p[i] = row[i];
                    }
            } else {
                int32_t *p = out_s + fc * och;
                const uint32_t nd = nfc * och;
                const Row r(p, nd);
                const uint32_t i = r.single(t, nd);
#pragma unroll 2
                for (uint32_t g0 = t; g0 < r.groups; g0 += THREADS) {
                    const uint32_t d = r.head + 4u * g0;
                    uint32_t f = div_small(d, och, inv_o), c = d - f * och;
                    int32_t v[4];
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) {
                        v[j] = s_buf[c * PITCH + f];
                        c++;
                        if (c == och)
                            c = 0, f++;
                    }
                    *reinterpret_cast<int4 *>(p + d) = make_int4(v[0], v[1], v[2], v[3]);
                }
                if (i < nd) {
                    const uint32_t f = div_small(i, och, inv_o);
                    p[i] = s_buf[(i - f * och) * PITCH + f];
                }
            }
            __syncthreads();            // (s_buf has been read: the next chunk fills it)
        }
        cnt.store(rec + (uint64_t)b * REC, s_red);
    }
}

// ---- step 4: one workgroup per stream sums the stream's records.  A stream whose tiles do not all lie inside the
//      caller's bound is reported as zeros, as one that is not taken.
__global__ __launch_bounds__(THREADS) void k_mix_join(const dvda_pcm_crc_desc *__restrict__ desc_in,
                                                      const dvda_pcm_crc_desc *__restrict__ desc_out,
                                                      const dvda_pcm_mix *__restrict__ mat, uint32_t n,
                                                      const uint32_t *__restrict__ base, const uint32_t *__restrict__ rec,
                                                      uint32_t max_tiles, dvda_pcm_mix_report *__restrict__ out)
{
    __shared__ uint64_t s_red[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= n)
        return;
    uint64_t frames = take(desc_in[s], desc_out[s], mat[s]);
    const uint32_t first = base[s], n_t = lvl::tiles_of(frames);
    if ((uint64_t)first + n_t > max_tiles)
        frames = 0;
    if (threadIdx.x == 0)
        out[s].frames = frames;
    pcmw::join_clipped(rec, first, frames ? n_t : 0u, frames ? desc_out[s].channels : 0u, s_red, out[s].clipped);
}

} // namespace mix
