// mlp_conceal.h -- conceal mode of the batch tier (dvda_mlp_hip_set_conceal): a damaged stream comes out as
//   kept PCM ++ silence ++ PCM of a fresh decoder from the next usable major sync ++ ...
// instead of being refused whole.  The reference asserts on the same damage (src/mlp.c:547, 566, 571, 756-798).
//
//   k_conceal_plan   one lane per damaged stream of an index: where its kept byte ranges begin and end
//   k_conceal_gather the ranges to decode again, copied into a 16-byte aligned workspace (a second index)
//   k_conceal_move   decoded ranges from their scratch to their place in the caller's buffer
//   k_conceal_fill   zeros for the concealed spans
// The host (mlp_conceal_run.h, conceal_run) decodes the ranges in rounds, each range a stream of its own with fresh state,
// and lays the result out; DESIGN.md section "Conceal mode" states the rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mlp_index.h"

namespace mlp {

// what makes a segment or a stream damaged: everything outside DVDA_ST_BENIGN except the capacity reports (OVERFLOW,
// CAPACITY: the caller's sizes, not the bytes) and DVDA_ST_ENVELOPE -- a fresh decoder that starts at a major sync whose
// first block continues the FIR history (DVDA_ST_CHAINED) reads history the reference never had there; it is decoded
// with zero history, as the oracle decodes it, and that is what conceal mode hands out
constexpr uint32_t CONCEAL_DAMAGE = 0x1FDu | (1u << 16);
// what the fast pass leaves to the sequential pass, which decodes a stream in order and stops at its first damage: behind
// that damage such a segment's status is all there is, and a damaged unit can be what made the segment look so
constexpr uint32_t CONCEAL_DEFERRED = (1u << 17) | (1u << 25);      // DVDA_ST_TIMING | DVDA_ST_SEQ
constexpr uint32_t CONCEAL_MAX_RANGES = 16;     // kept ranges one plan holds; a stream with more is planned again
                                                // from the last one in the next round
constexpr uint32_t CONCEAL_MAX_WALK = 1u << 20; // access units one walk over a damaged segment checks at most
constexpr uint32_t CONCEAL_ROUNDS = 4;          // decode rounds: the caller's batch, then up to three of kept ranges

struct ConcealRange {
    uint64_t a, b;          // kept byte range, relative to the stream's start
    uint32_t t_first;       // 16-bit input timing of the unit at a (the end of the range, t_k + n_k, is t_first + the PCM
                            // frames the range decodes to: the host adds them once the range is decoded)
    uint32_t cause;         // DVDA_ST_* bits of the damage in front of a (0: none)
    uint32_t last;          // 1: the plan stopped here (more ranges than CONCEAL_MAX_RANGES): b = the stream's end
    uint32_t pad;
};
struct ConcealPlan {
    uint32_t n;             // kept ranges
    uint32_t tail_cause;    // DVDA_ST_* bits of the damage behind the last range (0: it runs to the stream's end)
    uint32_t pad[2];
    ConcealRange r[CONCEAL_MAX_RANGES];
};

__device__ __forceinline__ uint32_t cc_u8(const uint8_t *b, uint64_t p) { return b[p]; }
__device__ __forceinline__ uint32_t cc_size(const uint8_t *b, uint64_t p)
{
    return 2u * (((cc_u8(b, p) & 0x0Fu) << 8) | cc_u8(b, p + 1));
}
__device__ __forceinline__ uint32_t cc_timing(const uint8_t *b, uint64_t p) { return (cc_u8(b, p + 2) << 8) | cc_u8(b, p + 3); }

// Framing and check data of the access unit at p of a stream that ends at lim, as reference src/mlp.c:407-468,
// 656-712 read them (oracle/mlp_oracle.c decode_frame, check_substream): 0 = the unit is framed and its substreams
// verify, else the DVDA_ST_* bit of the first thing that fails.  S = the stream's substream count.
__device__ uint32_t conceal_unit_check(const uint8_t *b, uint64_t p, uint64_t lim, uint32_t S)
{
    if (p + 4 > lim)
        return 1u << 4;
    const uint32_t size = cc_size(b, p);
    if (size < 4 || p + size > lim)
        return 1u << 4;
    const uint64_t fe = p + size;
    uint64_t q = p + 4;
    if (sync_frame_at(b, p, fe))
        q = p + 32;
    uint32_t end[2] = {0, 0}, check = 0;
    for (uint32_t s = 0; s < S; s++) {
        if (q + 2 > fe)
            return 1u << 4;
        const uint32_t w = (cc_u8(b, q) << 8) | cc_u8(b, q + 1);
        if (s == 0)
            check = (w >> 13) & 1u;         // substream 1 is checked with substream 0's flag (src/mlp.c:545)
        end[s] = (w & 0xFFFu) * 2u;
        q += (w & 0x8000u) ? 4u : 2u;
    }
    if (q > fe)
        return 1u << 4;
    uint32_t prev = 0;
    for (uint32_t s = 0; s < S; s++) {
        if (end[s] < prev || q + end[s] > fe || (check && end[s] - prev < 2u))
            return 1u << 4;
        if (check) {
            uint32_t parity = 0, crc = 0x3Cu, fin = 0;
            for (uint64_t k = q + prev; k + 2 < q + end[s]; k++) {
                const uint32_t v = cc_u8(b, k);
                parity ^= v;
                fin = crc ^ v;
                crc = fin;
#pragma unroll
                for (int t = 0; t < 8; t++)
                    crc = (crc & 0x80u) ? ((crc << 1) ^ 0x63u) & 0xFFu : (crc << 1) & 0xFFu;
            }
            if (((cc_u8(b, q + end[s] - 2) ^ parity) & 0xFFu) != 0xA9u)
                return 1u << 2;
            if (fin != cc_u8(b, q + end[s] - 1))
                return 1u << 3;
        }
        prev = end[s];
    }
    return 0;
}

// Can a fresh decoder start at p?  A major sync with the stream's parameters (`want`) whose every substream opens
// with a restart header (decode_block src/mlp.c:748-753; the same rule as dvda_disc.c win_unit_restarts), and whose
// unit is framed and verifies.
__device__ bool conceal_can_resume(const uint8_t *b, uint64_t p, uint64_t lim, uint32_t want)
{
    if (!sync_frame_at(b, p, lim) || ((packed_sync_at(b, p) ^ want) & SYNC_PARAMS) != 0)
        return false;
    const uint32_t S = cc_u8(b, p + 20) >> 4;
    const uint32_t size = cc_size(b, p);
    if (p + size > lim)
        return false;
    const uint64_t fe = p + size;
    uint64_t q = p + 32;
    uint32_t end0 = 0;
    for (uint32_t s = 0; s < S; s++) {
        if (q + 2 > fe)
            return false;
        const uint32_t w = (cc_u8(b, q) << 8) | cc_u8(b, q + 1);
        if (s == 0)
            end0 = (w & 0xFFFu) * 2u;
        q += (w & 0x8000u) ? 4u : 2u;
    }
    if (q >= fe || (cc_u8(b, q) & 0xC0u) != 0xC0u)
        return false;
    if (S == 2 && (q + end0 >= fe || (cc_u8(b, q + end0) & 0xC0u) != 0xC0u))
        return false;
    return conceal_unit_check(b, p, lim, S) == 0;
}

// One lane per stream of a decoded index; a stream whose status carries no damage bit leaves at once (plan.n = ~0).
// Walks the stream's segments from the first usable major sync: a damaged segment (its decode status) is searched unit by
// unit for the first unit that fails its own checks -- the range ends there -- or, when none does, ends the range at its
// major sync; then the next usable major sync behind the damage opens the next range.  Offsets relative to the stream.
__global__ __launch_bounds__(64) void k_conceal_plan(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ soff,
                                                     const uint64_t *__restrict__ slen, const SegRec *__restrict__ seg,
                                                     const uint32_t *__restrict__ seg_status,
                                                     const uint32_t *__restrict__ n_seg_ptr, uint32_t max_seg,
                                                     const StreamRec *__restrict__ streams, uint32_t n_streams,
                                                     ConcealPlan *__restrict__ plan)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams)
        return;
    const StreamRec sr = streams[s];
    ConcealPlan &P = plan[s];
    if (!(sr.status & CONCEAL_DAMAGE)) {
        P.n = 0xFFFFFFFFu;                  // not damaged: not planned
        return;
    }
    uint32_t n_cand = *n_seg_ptr;
    if (n_cand > max_seg)
        n_cand = max_seg;
    const uint64_t s_begin = soff[s], s_end = s_begin + slen[s];
    uint32_t n = 0, cause = 0;
    P.tail_cause = 0;
    if (sr.first_seg == 0xFFFFFFFFu || sr.first_seg >= n_cand) {
        // no major sync at all: nothing to keep
        P.n = 0;
        P.tail_cause = (sr.status & CONCEAL_DAMAGE) | 1u;
        return;
    }
    const uint32_t want = sr.sync & SYNC_PARAMS;
    const uint32_t S = (sr.sync >> 24) & 0xFu;
    uint64_t bound = s_begin;               // a fresh decoder may start at a candidate at or behind this offset
    uint32_t i = sr.first_seg;
    for (;;) {
        // ---- resume: the first usable major sync at or behind `bound` (dead candidates included: a walk through the
        //      damage may have passed over the real syncs behind it)
        uint32_t g = i;
        while (g < n_cand && seg[g].stream == s && !(seg[g].off >= bound && conceal_can_resume(bytes, seg[g].off, s_end, want)))
            g++;
        if (g >= n_cand || seg[g].stream != s) {
            if (bound < s_end)
                P.tail_cause = cause ? cause : (1u << 0);
            break;
        }
        if (seg[g].off > bound && n == 0 && cause == 0)
            cause = 1u << 0;                // bytes in front of the first usable major sync: DVDA_ST_NO_SYNC
        ConcealRange R;
        R.a = seg[g].off - s_begin;
        R.t_first = cc_timing(bytes, seg[g].off);
        R.cause = cause;
        R.last = 0;
        R.pad = 0;
        cause = 0;
        if (n + 1 == CONCEAL_MAX_RANGES) {
            // the last slot: this range runs to the end and is planned again after its own decode
            R.b = s_end - s_begin;
            R.last = 1;
            P.r[n++] = R;
            break;
        }
        // ---- walk the live segments of the range: the first damaged one ends it
        uint64_t kept_end = s_end;
        // (a range that starts behind damage was decoded with the state of the bytes in front of it -- a chain of segments
        //  that continue the FIR history carries a failure into every segment behind it: only the units' own checks say
        //  anything there; the range's decode is judged again, fresh, in the next round)
        const bool fresh = seg[g].off != s_begin;
        uint32_t h = g;
        for (; h < n_cand && seg[h].stream == s; h++) {
            const SegRec r = seg[h];
            if (r.off < seg[g].off || ((r.flags & SEG_DEAD) && h != g))
                continue;
            uint32_t nxt = h + 1;
            while (nxt < n_cand && seg[nxt].stream == s && (seg[nxt].flags & SEG_DEAD))
                nxt++;
            const uint64_t lim = (nxt < n_cand && seg[nxt].stream == s) ? seg[nxt].off : s_end;
            const uint32_t st = (seg_status[h] | r.flags) & ~SEG_DEAD;
            // (behind damage the units of a segment left to the sequential pass are checked like those of one that reports
            //  damage: CONCEAL_DEFERRED)
            const bool damaged = fresh ? (st & ((CONCEAL_DAMAGE & ~(1u << 0)) | CONCEAL_DEFERRED)) != 0
                                       : (st & CONCEAL_DAMAGE) != 0;
            if (damaged) {
                uint64_t p = r.off;
                uint32_t fail = 0;
                for (uint32_t k = 0; k < CONCEAL_MAX_WALK && p < s_end; k++) {
                    fail = conceal_unit_check(bytes, p, s_end, S);
                    if (fail)
                        break;
                    p += cc_size(bytes, p);
                    if (p == lim)
                        break;
                }
                if (fail) {
                    kept_end = p;
                    cause = fail | (st & CONCEAL_DAMAGE);
                    break;
                }
                if (!fresh) {
                    // nothing the units say: the segment's decode failed -- the whole segment is damaged
                    kept_end = r.off;
                    cause = st & CONCEAL_DAMAGE;
                    break;
                }
            }
        }
        R.b = kept_end - s_begin;
        if (R.b > R.a) {
            P.r[n++] = R;
        } else {
            cause |= R.cause;               // nothing kept: the damage in front of it and behind it are one span
        }
        if (kept_end >= s_end)
            break;
        bound = kept_end + 2;
        i = g + 1;
    }
    P.n = n;
}

// the ranges to decode again, into a 16-byte aligned workspace: piece k = src[src_off[k] .. + len[k]) ->
// dst[dst_off[k] ..).  A workgroup per piece; 16-bit copies (pieces start at even offsets).
__global__ __launch_bounds__(256) void k_conceal_gather(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        const uint64_t *__restrict__ tab, uint32_t n_pieces)
{
    for (uint32_t k = blockIdx.y; k < n_pieces; k += gridDim.y) {
        const uint64_t so = tab[3 * k], d = tab[3 * k + 1], len = tab[3 * k + 2];
        const uint16_t *s16 = reinterpret_cast<const uint16_t *>(src + so);
        uint16_t *d16 = reinterpret_cast<uint16_t *>(dst + d);
        for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len / 2; e += (uint64_t)gridDim.x * blockDim.x)
            d16[e] = s16[e];
        if ((len & 1) && blockIdx.x == 0 && threadIdx.x == 0)
            dst[d + len - 1] = src[so + len - 1];
    }
}

// One placement: `frames` PCM frames of a stream with `channels` channels go to PCM frame `first` of the stream
// whose output starts at int32 offset dst_off of the caller's buffer (capacity / channel stride `stride` frames);
// they come from int32 offset src_off of a scratch buffer laid out the same way, channel stride src_stride (ZERO: zeros).
struct ConcealOp {
    uint64_t dst_off, src_off, first, frames, stride, src_stride;
    uint32_t channels, src;     // src: which scratch buffer (k_conceal_move)
};

// layout: 0 planar, 1 interleaved, 2 / 3 the WAV payload (3 / 2 bytes per value)
template <bool ZERO>
__device__ __forceinline__ void conceal_place(const ConcealOp &o, uint32_t layout, int32_t *__restrict__ pcm,
                                              const int32_t *__restrict__ src)
{
    const uint64_t C = o.channels;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (layout == 0) {
        const uint64_t n = o.frames * C;
        for (uint64_t e = t0; e < n; e += step) {
            const uint64_t c = e / o.frames, f = e % o.frames;
            pcm[o.dst_off + c * o.stride + o.first + f] = ZERO ? 0 : src[o.src_off + c * o.src_stride + f];
        }
    } else if (layout == 1) {
        const uint64_t n = o.frames * C;
        for (uint64_t e = t0; e < n; e += step)
            pcm[o.dst_off + o.first * C + e] = ZERO ? 0 : src[o.src_off + e];
    } else {
        // the payload starts at byte 4 * dst_off; a piece may start at any byte: byte stores
        const uint64_t nb = layout == 2 ? 3 : 2;
        const uint64_t n = o.frames * C * nb;
        uint8_t *d8 = reinterpret_cast<uint8_t *>(pcm) + 4 * o.dst_off + o.first * C * nb;
        const uint8_t *s8 = reinterpret_cast<const uint8_t *>(src) + 4 * o.src_off;
        for (uint64_t e = t0; e < n; e += step)
            d8[e] = ZERO ? 0 : s8[e];
    }
}

struct ConcealSrc {
    const int32_t *p[8];
};

// FIR history behind the last access unit of every stream of a decoded index (dvda_mlp_hip_conceal_edges: the streams are
// the kept ranges of a round): a workgroup per stream finds its last live segment and gathers that segment's column of
// the decode's FIR workspace -- element e of lane l = segment * 2 + substream lives at fir[e * lanes + l] -- into
// out[stream][substream][48], the layout of dvda_mlp_hip_segment_fir.  A stream without a live segment gets zeros.
__global__ __launch_bounds__(128) void k_conceal_edge_fir(const SegRec *__restrict__ seg, const uint32_t *__restrict__ n_seg_ptr,
                                                          uint32_t max_seg, const StreamRec *__restrict__ streams,
                                                          uint32_t n_streams, const int32_t *__restrict__ fir, uint32_t lanes,
                                                          int32_t *__restrict__ out)
{
    __shared__ uint32_t s_last;
    const uint32_t q = blockIdx.x;
    if (q >= n_streams)
        return;
    if (threadIdx.x == 0) {
        uint32_t n_cand = *n_seg_ptr, last = 0xFFFFFFFFu;
        if (n_cand > max_seg)
            n_cand = max_seg;
        for (uint32_t h = streams[q].first_seg; h < n_cand && seg[h].stream == q; h++)
            if (!(seg[h].flags & SEG_DEAD))
                last = h;
        s_last = last;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t >= 96)
        return;
    const uint64_t lane = (uint64_t)s_last * 2 + t / 48;
    const bool have = fir != nullptr && s_last != 0xFFFFFFFFu && lane < lanes;
    out[(size_t)q * 96 + t] = have ? fir[(size_t)(t % 48) * lanes + lane] : 0;
}

__global__ __launch_bounds__(256) void k_conceal_move(const ConcealOp *__restrict__ ops, uint32_t n_ops, uint32_t layout,
                                                      int32_t *__restrict__ pcm, ConcealSrc srcs)
{
    for (uint32_t k = blockIdx.y; k < n_ops; k += gridDim.y) {
        const ConcealOp o = ops[k];
        conceal_place<false>(o, layout, pcm, srcs.p[o.src & 7u]);
    }
}

__global__ __launch_bounds__(256) void k_conceal_fill(const ConcealOp *__restrict__ ops, uint32_t n_ops, uint32_t layout,
                                                      int32_t *__restrict__ pcm)
{
    for (uint32_t k = blockIdx.y; k < n_ops; k += gridDim.y) {
        const ConcealOp o = ops[k];
        conceal_place<true>(o, layout, pcm, nullptr);
    }
}

} // namespace mlp
