// mlp_present.h -- the 2-channel presentation of two-substream MLP (dvda_mlp_hip_set_presentation, DVDA_PRESENT_SUBSTREAM0).
//
// Substream 0 of a two-substream stream is a complete stream of its own: own restart headers, filters, matrices and
// output shifts (reference src/mlp.c:748-753, 822-826); a 2-channel decoder reads it alone.  These kernels make that
// stream out of the source -- the *presentation stream*: per complete access unit the frame header with the new
// length, the major sync with substream count 1 and the identity assignment of k channels, substream 0's directory
// word(s) and substream 0's bytes; substream 1's directory word(s) and bytes are left out.  What comes out is an
// ordinary one-substream stream (reference src/mlp.c:504-538), indexed and decoded by the kernels that are there.
//
//   k_pp_streams : one lane per stream -- k from the first unit's restart header, or why there is no presentation
//   k_pp_size    : one lane per live source segment walks its size chain and adds up the stripped size
//   (exclusive scan over the segments, k_pp_len, exclusive scan over the streams: every stream starts 16-byte aligned)
//   k_pp_fill    : the streams' ranges as the second index reads them; padding and the unused tail zeroed
//   k_pp_copy    : one wave per source segment -- rewritten headers as halfwords, bodies as 16-byte stores on the
//                  destination's alignment, the 2-byte aligned source shifted into place from two aligned loads
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mlp_index.h"

namespace mlp {

constexpr uint32_t PP_K_MASK = 0xFu;        // pp_info: k (0: a one-substream stream, copied as it is)
constexpr uint32_t PP_ENVELOPE = 1u << 8;   // two substreams, but no k: the first unit's substream 0 opens with no restart header
constexpr uint32_t PP_NONE = 1u << 9;       // the source index could not frame the stream: nothing is handed on
// source findings after which a stream is not decoded at all: DVDA_ST_NO_SYNC | DVDA_ST_IRREGULAR | DVDA_ST_CAPACITY
constexpr uint32_t PP_UNFRAMED = (1u << 0) | (1u << 16) | (1u << 22);

// one access unit of a two-substream stream, as offsets from its first byte
struct PpUnit {
    uint32_t sync;      // 28 when the unit carries a major sync, else 0
    uint32_t dir;       // bytes of substream 0's directory word(s): 0 (the unit ends before it), 2 or 4
    uint32_t body;      // first byte of the substream area
    uint32_t blen;      // bytes of substream 0 in it, clamped to the unit
    uint32_t out;       // bytes of the stripped unit = 4 + sync + dir + blen
};

__device__ __forceinline__ uint32_t pp_be16(const uint8_t *b, uint64_t p)
{
    const uint32_t v = *reinterpret_cast<const uint16_t *>(b + p);      // p is even
    return ((v & 0xFFu) << 8) | (v >> 8);
}

// the unit of `size` bytes at even offset p (hdr = its first 8 bytes, ld_hdr8)
__device__ __forceinline__ PpUnit pp_unit(const uint8_t *__restrict__ b, uint64_t p, uint32_t size, uint64_t hdr)
{
    PpUnit u;
    u.sync = 0;
    if (size >= 32 && (uint32_t)(hdr >> 32) == 0xBB6F72F8u) {
        const uint32_t count = ld_u8(b, p + 20) >> 4;
        if (count == 1 || count == 2)
            u.sync = 28;
    }
    uint32_t q = 4 + u.sync, end0 = 0;
    u.dir = 0;
    if (q + 2 <= size) {
        const uint32_t w0 = pp_be16(b, p + q);
        end0 = (w0 & 0xFFFu) * 2;
        u.dir = (w0 & 0x8000u) ? 4u : 2u;
        if (u.dir > size - q)
            u.dir = size - q;
        q += u.dir;
        if (q + 2 <= size) {
            const uint32_t w1 = pp_be16(b, p + q);
            const uint32_t n1 = (w1 & 0x8000u) ? 4u : 2u;
            q += n1 > size - q ? size - q : n1;
        }
    }
    u.body = q;
    u.blen = end0 < size - q ? end0 : size - q;
    u.out = 4 + u.sync + u.dir + u.blen;
    return u;
}

__device__ __forceinline__ uint32_t pp_au_size(uint64_t hdr)
{
    return 2u * ((((uint32_t)hdr & 0x0Fu) << 8) | (((uint32_t)hdr >> 8) & 0xFFu));
}

__global__ __launch_bounds__(256) void k_pp_streams(const uint8_t *__restrict__ bytes, const SegRec *__restrict__ seg,
                                                    const StreamRec *__restrict__ streams, uint32_t n_streams,
                                                    uint32_t max_seg, uint32_t *__restrict__ info)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams)
        return;
    const StreamRec r = streams[s];
    uint32_t v;
    if (r.first_seg >= max_seg || r.n_seg == 0 || (r.status & PP_UNFRAMED)) {
        v = PP_NONE;
    } else if (((r.sync >> 24) & 0xFu) != 2u) {
        v = 0;
    } else {
        v = PP_ENVELOPE;
        const SegRec g = seg[r.first_seg];
        if (g.nframes) {
            const uint64_t hdr = ld_hdr8(bytes, g.off);
            const uint32_t size = pp_au_size(hdr);
            if (size >= 4 && g.off + size <= g.end) {
                const PpUnit u = pp_unit(bytes, g.off, size, hdr);
                // both leading flags of the first block (parameters present, restart header present); behind them 13
                // bits of sync, the noise type, 16 bits of timestamp, min / max channel: bits 40-43 = max_matrix_channel
                if (u.blen >= 6 && (ld_u8(bytes, g.off + u.body) & 0xC0u) == 0xC0u) {
                    const uint32_t k = (ld_u8(bytes, g.off + u.body + 5) >> 4) + 1u;
                    if (k <= 5)
                        v = k;
                }
            }
        }
    }
    info[s] = v;
}

__global__ __launch_bounds__(256) void k_pp_size(const uint8_t *__restrict__ bytes, const SegRec *__restrict__ seg,
                                                 const uint32_t *__restrict__ n_seg_ptr, uint32_t max_seg,
                                                 const uint32_t *__restrict__ info, uint32_t *__restrict__ seg_size)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n = *n_seg_ptr;
    if (n > max_seg)
        n = max_seg;
    if (i >= n)
        return;
    const SegRec r = seg[i];
    const uint32_t v = info[r.stream];
    uint32_t total = 0;
    if (!(r.flags & SEG_DEAD) && r.nframes && !(v & (PP_NONE | PP_ENVELOPE))) {
        if ((v & PP_K_MASK) == 0) {
            total = (uint32_t)(r.end - r.off);
        } else {
            uint64_t p = r.off;
            for (uint32_t f = 0; f < r.nframes; f++) {
                const uint64_t hdr = ld_hdr8(bytes, p);
                const uint32_t size = pp_au_size(hdr);
                if (size < 4 || p + size > r.end)
                    break;                          // (cannot happen: the index walked this chain)
                total += pp_unit(bytes, p, size, hdr).out;
                p += size;
            }
        }
    }
    seg_size[i] = total;
}

// per stream: the presentation stream's length, and that length rounded up to the alignment of the next stream's start
__global__ __launch_bounds__(256) void k_pp_len(const StreamRec *__restrict__ streams, uint32_t n_streams,
                                                const uint32_t *__restrict__ n_seg_ptr, uint32_t max_seg,
                                                const uint32_t *__restrict__ info, const uint32_t *__restrict__ seg_base,
                                                uint32_t *__restrict__ len_pad, uint64_t *__restrict__ len64)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams)
        return;
    uint32_t n = *n_seg_ptr;
    if (n > max_seg)
        n = max_seg;
    const StreamRec r = streams[s];
    uint32_t len = 0;
    if (!(info[s] & (PP_NONE | PP_ENVELOPE)) && r.first_seg < n && r.n_seg <= n - r.first_seg)
        len = seg_base[r.first_seg + r.n_seg] - seg_base[r.first_seg];
    len_pad[s] = (len + 15u) & ~15u;
    len64[s] = len;
}

// the ranges the second index reads (on the device: the host does not wait in between), the few bytes between a
// stream's end and the next stream's start, and everything behind the last stream up to what the second index scans:
// zeros, so that no byte of an earlier batch is taken for a major sync
__global__ __launch_bounds__(256) void k_pp_fill(uint8_t *__restrict__ out, uint64_t out_bytes, uint32_t n_streams,
                                                 const uint32_t *__restrict__ base, const uint64_t *__restrict__ len64,
                                                 uint64_t *__restrict__ off64)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_streams) {
        const uint64_t o = base[t], l = len64[t];
        off64[t] = o;
        for (uint64_t q = o + l; q < ((o + l + 15u) & ~(uint64_t)15u); q += 2)      // (lengths are even)
            *reinterpret_cast<uint16_t *>(out + q) = 0;
    }
    const uint64_t used = base[n_streams];          // a multiple of 16
    const uint64_t o = t * 16;
    if (o >= used && o + 16 <= out_bytes)
        *reinterpret_cast<uint4 *>(out + o) = make_uint4(0, 0, 0, 0);
}

template <int DS, bool HALF>
__device__ __forceinline__ uint4 pp_shift(const uint4 A, const uint4 B)
{
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        o[j] = HALF ? ((w[DS + j] >> 16) | (w[DS + j + 1] << 16)) : w[DS + j];
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// n bytes (even) from src to dst (both 2-byte aligned) by the 64 lanes of a wave: halfwords up to dst's next 16-byte
// boundary, 16-byte stores from there, halfwords for what is left.  The source of a 16-byte store is two aligned
// 16-byte loads shifted by the (wave-uniform) distance between the two alignments; the second load reads at most 30
// bytes past src + n (the input buffers are readable 64 bytes past their end).
__device__ __forceinline__ void pp_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t n, uint32_t lane)
{
    uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    if (head > n)
        head = n;
    if (lane < head / 2)
        reinterpret_cast<uint16_t *>(dst)[lane] = reinterpret_cast<const uint16_t *>(src)[lane];
    dst += head;
    src += head;
    n -= head;
    const uint32_t chunks = n >> 4;
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src - a);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    if (a == 0) {
        for (uint32_t c = lane; c < chunks; c += 64)
            d4[c] = s4[c];
    } else {
        for (uint32_t c = lane; c < chunks; c += 64) {
            const uint4 A = s4[c], B = s4[c + 1];
            uint4 v;
            switch (a >> 1) {
            case 1: v = pp_shift<0, true>(A, B); break;
            case 2: v = pp_shift<1, false>(A, B); break;
            case 3: v = pp_shift<1, true>(A, B); break;
            case 4: v = pp_shift<2, false>(A, B); break;
            case 5: v = pp_shift<2, true>(A, B); break;
            case 6: v = pp_shift<3, false>(A, B); break;
            default: v = pp_shift<3, true>(A, B); break;
            }
            d4[c] = v;
        }
    }
    const uint32_t tail = (n & 15u) / 2;
    if (lane < tail)
        reinterpret_cast<uint16_t *>(dst + 16 * (size_t)chunks)[lane] =
            reinterpret_cast<const uint16_t *>(src + 16 * (size_t)chunks)[lane];
}

constexpr int PP_THREADS = 256;

// One wave per source segment (waves stride over the segments).  out + base[stream] + (seg_base[i] - seg_base[first
// segment of the stream]) is where segment i's stripped bytes go; nothing is written past seg_size[i] of them.
__global__ __launch_bounds__(PP_THREADS) void k_pp_copy(const uint8_t *__restrict__ bytes, const SegRec *__restrict__ seg,
                                                        const uint32_t *__restrict__ n_seg_ptr, uint32_t max_seg,
                                                        const StreamRec *__restrict__ streams,
                                                        const uint32_t *__restrict__ info,
                                                        const uint32_t *__restrict__ seg_size,
                                                        const uint32_t *__restrict__ seg_base,
                                                        const uint32_t *__restrict__ base, uint8_t *__restrict__ out)
{
    uint32_t n = *n_seg_ptr;
    if (n > max_seg)
        n = max_seg;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (PP_THREADS / 64);
    for (uint32_t i = blockIdx.x * (PP_THREADS / 64) + (threadIdx.x >> 6); i < n; i += waves) {
        const uint32_t size = seg_size[i];
        if (size == 0)
            continue;
        const SegRec r = seg[i];
        const uint32_t k = info[r.stream] & PP_K_MASK;
        uint8_t *dst = out + base[r.stream] + (seg_base[i] - seg_base[streams[r.stream].first_seg]);
        if (k == 0) {
            pp_copy(dst, bytes + r.off, size, lane);
            continue;
        }
        // identity assignment of k channels: MLP channel c is RIFF channel c (reference src/mlp.c:416-438)
        const uint32_t ident = k == 5 ? 0x06u : k - 1u;
        uint8_t *const dst_end = dst + size;
        uint64_t p = r.off;
        for (uint32_t f = 0; f < r.nframes; f++) {
            const uint64_t hdr = ld_hdr8(bytes, p);
            const uint32_t au = pp_au_size(hdr);
            if (au < 4 || p + au > r.end)
                break;
            const PpUnit u = pp_unit(bytes, p, au, hdr);
            if (dst + u.out > dst_end)
                break;                              // (cannot happen: k_pp_size added up the same units)
            // frame header, major sync and directory: one halfword per lane
            const uint32_t hs = u.sync / 2, hw = 2 + hs + u.dir / 2;
            if (lane < hw) {
                uint32_t v;
                if (lane == 0) {
                    const uint32_t words = u.out / 2;
                    v = (((uint32_t)hdr & 0xF0u) | (words >> 8)) | ((words & 0xFFu) << 8);
                } else if (lane == 1) {
                    v = (uint32_t)(hdr >> 16) & 0xFFFFu;
                } else if (lane < 2 + hs) {
                    v = *reinterpret_cast<const uint16_t *>(bytes + p + 2 * (uint64_t)lane);
                    if (lane == 5)                  // unit byte 11: the 5-bit channel assignment
                        v = (v & 0xE0FFu) | (ident << 8);
                    if (lane == 10)                 // unit byte 20: the substream count
                        v = (v & 0xFF0Fu) | 0x0010u;
                } else {
                    v = *reinterpret_cast<const uint16_t *>(bytes + p + 4 + u.sync + 2 * (uint64_t)(lane - 2 - hs));
                }
                reinterpret_cast<uint16_t *>(dst)[lane] = (uint16_t)v;
            }
            pp_copy(dst + 2 * hw, bytes + p + u.body, u.blen, lane);
            dst += u.out;
            p += au;
        }
    }
}

} // namespace mlp
