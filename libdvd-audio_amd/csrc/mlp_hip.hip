// mlp_hip.hip -- the one translation unit of the library: the batch core's C-ABI entry points
// (include/dvda_mlp_hip.h: create / destroy, index, reserve, decode, the setters, the getters, the
// self-tests) and the launch sequence of the gfx950 kernels.
//
//   index : k_sync_mask -> k_exscan_u32 -> k_sync_scatter -> k_chase ->
//           k_exscan_u32 -> k_link                 (framing, src/mlp.c:384-405)
//           -> k_au_check                          (parity / CRC-8 of every substream, src/mlp.c:670-712)
//   decode: k_decode (fast pass) -> k_finalize -> [summary to the host] ->
//           chain passes (mlp_chain.h) and / or the sequential pass, only when the fast pass
//           left something to them                 (src/mlp.c:407-1358)
//
// The index does no allocation and no host synchronisation.  The decode waits once for the fast
// pass (a 32-byte summary decides what else is launched); a batch with chained segments grows the
// chain workspace on first use.
//
// Host code beside the core, each in a header included here: hip_ws.h (owning buffers and handles), mlp_ctx.h (the
// context), mlp_conceal_run.h, mlp_present_run.h (the two modes), mlp_stepper.h (streaming tier), mlp_tiers.h (raw PCM,
// demux, WAV payload), pcm_report_run.h (the reports of the decoded PCM: its CRC-32, its levels, its compare with another buffer,
// its energy, its reduction to a smaller word length, its decimation by 2 or 4, 48 kHz resampled to 44.1 kHz, and its
// channel mix).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

#include "../../include/dvda_mlp_hip.h"
#include "mlp_step.h"
#include "mlp_decode.h"
#include "mlp_chain.h"
#include "mlp_chain_small.h"
#include "mlp_check.h"
#include "mlp_coop.h"
#include "mlp_index.h"
#include "mlp_conceal.h"
#include "mlp_present.h"
#include "pcm_unswizzle.h"
#include "wav_pack.h"
#include "pcm_digest.h"
#include "pcm_levels.h"
#include "pcm_compare.h"

#include "mlp_ctx.h"
#include "mlp_conceal_run.h"
#include "mlp_present_run.h"
#include "mlp_stepper.h"
#include "mlp_tiers.h"
#include "pcm_report_run.h"

// range-checked build: violations counted by the kernels so far (0 in the shipped library, which does not check)
extern "C" int dvda_mlp_hip_bounds_violations(unsigned long long *out4)
{
    if (!out4)
        return DVDA_HIP_EINVAL;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
#if defined(DVDA_BOUNDS)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out4, HIP_SYMBOL(mlp::g_bounds), 4 * sizeof(unsigned long long)));
    return 1;       // (a checked build)
#else
    return DVDA_HIP_OK;
#endif
}

extern "C" const char *dvda_mlp_hip_version(void) { return "dvda-mlp-hip 0.1 (gfx950)"; }

extern "C" int dvda_mlp_hip_create(dvda_mlp_hip_ctx **out, int device, uint32_t max_streams,
                                   uint32_t max_segments)
{
    if (!out || max_streams == 0 || max_segments == 0)
        return DVDA_HIP_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        fprintf(stderr, "dvda_mlp_hip: no usable HIP device (count=%d, requested=%d)\n", ndev, device);
        return DVDA_HIP_ENODEV;
    }
    HIP_TRY(hipSetDevice(device));
    dvda_mlp_hip_ctx *c = new (std::nothrow) dvda_mlp_hip_ctx();       // (every field zero, or its default)
    if (!c)
        return DVDA_HIP_ENOMEM;
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
            cus = 256;
        c->coop_min_seg = (uint32_t)cus * 4u * 64u * 7u / 4u;
        if (const char *e = getenv("DVDA_COOP_MIN_SEG"))
            c->coop_min_seg = (uint32_t)strtoul(e, nullptr, 10);
    }
    c->max_streams = max_streams;
    c->max_segments = max_segments;
    c->idx_graph_state = getenv("DVDA_INDEX_GRAPH") && atoi(getenv("DVDA_INDEX_GRAPH")) == 0 ? -1 : 0;
    const size_t ns = (size_t)max_segments, nt = (size_t)max_streams;
    // two lanes per segment at most, rounded up to whole workgroups
    c->iir_lanes = (uint32_t)(((2 * ns + DEC_THREADS - 1) / DEC_THREADS) * DEC_THREADS);
    const size_t nl = c->iir_lanes;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &buf, size_t n) {
        if (e == hipSuccess)
            e = buf.alloc(n);
    };
    alloc(c->d_cand_off, ns);
    // (+ 4 entries on the arrays k_chain_fused prefetches 16 bytes at a time from: the read behind the last index stays inside)
    alloc(c->d_seg, ns + 4);
    alloc(c->d_seg_frames, ns + 1);
    alloc(c->d_seg_fbase, ns + 5);
    alloc(c->d_seg_status, ns + 4);
    alloc(c->d_seg_rows, ns);
    alloc(c->d_streams, nt);
    alloc(c->d_iir, nl * MAXCH * 16);
    alloc(c->d_mat, nl * MAXMAT * 5);
    alloc(c->d_dbg, 32);
    alloc(c->d_fir, nl * 6 * 8);
    alloc(c->d_seg_meta, nl + 4);
    alloc(c->d_yield, ns);
    alloc(c->d_seg_check, 2 * ns);
    alloc(c->d_cls, 4);
    alloc(c->d_shape_key, nt);
    alloc(c->d_soff, nt);
    alloc(c->d_slen, nt);
    alloc(c->d_rank, nt);
    alloc(c->d_sorted_cnt, nt + 1);
    alloc(c->d_sorted_base, nt + 1);
    alloc(c->d_lane_seg, ns);
    alloc(c->d_summary, 1 + SUMMARY_PARTS);         // the total + the fast pass's partial sums
    alloc(c->d_seq_list, nt);
    alloc(c->d_plan, ns + 5);
    alloc(c->d_scan4_tmp, ns / 1024 + 4);
    alloc(c->d_def_list, ns);
    alloc(c->d_head_list, ns);
    alloc(c->d_chain_order, ns);
    alloc(c->d_chain_hist, 2 * CHAIN_BUCKETS);
    if (e == hipSuccess)
        e = hipHostMalloc((void **)&c->h_summary, sizeof(DecodeSummary), hipHostMallocDefault);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(c->st_aux.put(), hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(c->ev_fork.put(), hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(c->ev_join.put(), hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipMemset(c->d_dbg, 0, 32 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemset(c->d_seg_meta, 0, nl * sizeof(uint32_t));
    // the event ring is made here: the decode calls create nothing
    for (uint32_t i = 0; e == hipSuccess && i < 2 * EV_RING; i++)
        e = hipEventCreate(c->ev[i].put());
    for (uint32_t i = 0; e == hipSuccess && i < EV_RING; i++)
        e = hipEventCreate(c->ev_end[i].put());
    if (e != hipSuccess) {
        fprintf(stderr, "dvda_mlp_hip: workspace allocation failed: %s\n", hipGetErrorString(e));
        delete c;
        return DVDA_HIP_ENOMEM;
    }
    *out = c;
    return DVDA_HIP_OK;
}

extern "C" void dvda_mlp_hip_destroy(dvda_mlp_hip_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
#if defined(DVDA_BOUNDS)
    if (getenv("DVDA_BOUNDS_REPORT")) {
        unsigned long long v[4] = {0, 0, 0, 0};
        (void)dvda_mlp_hip_bounds_violations(v);
        fprintf(stderr, "dvda_mlp_hip: bounds violations: %llu", v[0]);
        if (v[0])
            fprintf(stderr, " (first: tag %llu index %llu capacity %llu)", v[1], v[2], v[3]);
        fprintf(stderr, "\n");
    }
#endif
    delete c;       // (its members free what they hold, the modes' child contexts included)
}

// byte-proportional workspace grows on demand OUTSIDE the timed path: the first
// index call for a larger batch (re)allocates, later calls of the same size reuse
static int ensure_byte_ws(dvda_mlp_hip_ctx *c, uint64_t total_bytes)
{
    const uint64_t chunks = (total_bytes + 15) / 16 + 4;
    const uint64_t tiles = (chunks + IDX_TILE_CHUNKS - 1) / IDX_TILE_CHUNKS;
    // two buffers that go by the capacity of the first: both are let go before either is allocated anew, and a
    // pair of which one is missing counts as none
    auto grow_pair = [](auto &a, uint64_t na, auto &b, uint64_t nb) {
        if (na <= a.cap)
            return DVDA_HIP_OK;
        a.release();
        b.release();
        if (a.alloc(na) == hipSuccess && b.alloc(nb) == hipSuccess)
            return DVDA_HIP_OK;
        a.release();
        return DVDA_HIP_ENOMEM;
    };
    int rc = grow_pair(c->d_masks, chunks, c->d_parts, chunks + 72);
    if (rc)
        return rc;
    uint64_t most = tiles > c->max_segments ? tiles : c->max_segments;
    if (c->max_streams > most)
        most = c->max_streams;
    if ((rc = c->d_scan_tmp.grow_exact((most + 1023) / 1024 + 2)) != 0)
        return rc;
    // (d_tile_count's capacity is tiles + 1: the comparison is the one `tiles > capacity in tiles` was)
    return grow_pair(c->d_tile_count, tiles + 1, c->d_tile_base, tiles + 1);
}

// one dispatch for the things an index call starts from: empty stream records, and the per-segment status /
// row counters / end-of-segment notes at zero (a note of the batch before must not vouch for a segment of this one)
__global__ void k_init_streams(StreamRec *s, uint32_t n, uint32_t *seg_status, uint32_t *seg_rows, uint32_t *yield_req,
                               uint32_t *seg_meta, uint32_t n_seg, uint32_t *cls, uint32_t *summary_words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4)
        cls[i] = 0;                 // substream classes, "the batch mixes shapes" (a memset of its own cost a launch)
    // the decode summary and its partial sums start from zero: the first decode call on this index finds them so
    // (its own memset was a launch and a host gap in front of the fast pass: 13 us of a small batch's 165)
    if (i < (1 + SUMMARY_PARTS) * sizeof(DecodeSummary) / sizeof(uint32_t))
        summary_words[i] = 0;
    if (i < n_seg) {
        seg_status[i] = 0;
        seg_rows[i] = 0;
        yield_req[i] = 0;
        seg_meta[2 * (size_t)i] = seg_meta[2 * (size_t)i + 1] = 0;
    }
    if (i < n) {
        StreamRec r;
        r.first_seg = 0xFFFFFFFFu;
        r.n_seg = 0;
        r.sync = 0;
        r.status = 0;
        r.frames = 0;
        r.consumed = 0;
        r.rows = 0;
        s[i] = r;
    }
}

// A decode call on an index that has been decoded before (the caller came back with a larger PCM buffer, say):
// what the decode passes left on the segments -- status bits, row counts, yield requests, end-of-segment notes --
// goes back to what the index left, or the second decode would take the first one's findings for its own.
__global__ void k_reset_segments(uint32_t *seg_status, uint32_t *seg_rows, uint32_t *yield_req, uint32_t *seg_meta,
                                 uint32_t n_seg)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seg) {
        seg_status[i] = 0;
        seg_rows[i] = 0;
        yield_req[i] = 0;
        seg_meta[2 * (size_t)i] = seg_meta[2 * (size_t)i + 1] = 0;
    }
}

// The index looks streams up by offset (find_stream: the last stream that starts at or before a byte) and takes a
// stream's segments to be neighbours in the list of major syncs: the caller's ranges have to be ascending, disjoint,
// 16-byte aligned and inside the buffer.  Checked here, on the device, instead of trusted: a stream whose range
// starts before the end of any stream in front of it, is misaligned or leaves the buffer gets length 0 (nothing of
// it is decoded) and DVDA_ST_IRREGULAR | DVDA_ST_ENVELOPE, and the offsets the index works with are made ascending (max with the
// furthest end so far) whatever the caller passed.  One workgroup: a running maximum over the streams in order.
__device__ __forceinline__ void check_ranges_block(const uint64_t *__restrict__ off, const uint64_t *__restrict__ len,
                                                   uint32_t n, uint64_t total_bytes, uint64_t *__restrict__ soff,
                                                   uint64_t *__restrict__ slen, StreamRec *__restrict__ streams,
                                                   unsigned long long *s_max)
{
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    auto end_of = [&](uint32_t i) {
        const uint64_t o = off[i], l = len[i];
        return (o <= total_bytes && l <= total_bytes - o && (o & 15u) == 0) ? o + l : 0;   // (a range that is refused
    };                                                                                     //  stands in nobody's way)
    unsigned long long m = 0;
    for (uint32_t i = lo; i < hi; i++) {
        const unsigned long long e = end_of(i);
        m = e > m ? e : m;
    }
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {          // inclusive running maximum over the 1024 parts
        const unsigned long long v = threadIdx.x >= d ? s_max[threadIdx.x - d] : 0ull;
        __syncthreads();
        if (v > s_max[threadIdx.x])
            s_max[threadIdx.x] = v;
        __syncthreads();
    }
    unsigned long long run = threadIdx.x ? s_max[threadIdx.x - 1] : 0ull;           // furthest end in front of part lo
    for (uint32_t i = lo; i < hi; i++) {
        const uint64_t o = off[i], l = len[i];
        const bool ok = (o & 15u) == 0 && o <= total_bytes && l <= total_bytes - o && o >= run;
        // (a refused stream becomes an empty range where the ascending order wants it: the streams behind it keep
        //  theirs -- ONE bad entry does not cost the rest of the batch)
        const uint64_t so = ok ? o : run;
        soff[i] = so < total_bytes ? so : total_bytes;
        slen[i] = ok ? l : 0;
        if (!ok)
            streams[i].status = ST_ENVELOPE | (1u << 16);       // (+ DVDA_ST_IRREGULAR: an index finding, kept by k_finalize)
        const unsigned long long e = end_of(i);
        run = e > run ? e : run;
    }
}

__global__ __launch_bounds__(1024) void k_check_ranges(const uint64_t *__restrict__ off, const uint64_t *__restrict__ len,
                                                       uint32_t n, uint64_t total_bytes, uint64_t *__restrict__ soff,
                                                       uint64_t *__restrict__ slen, StreamRec *__restrict__ streams)
{
    __shared__ unsigned long long s_max[1024];
    check_ranges_block(off, len, n, total_bytes, soff, slen, streams, s_max);
}

// An input of at most SMALL_INPUT_BYTES is decoded by the cooperative kernel whatever the index finds in it (the lane
// kernels' two launches -- 9 us of early exits -- are not even enqueued).
// (Tried in round 3 and removed: the index of such an input as ONE workgroup of 1 024 threads running every phase
//  behind k_sync_mask with barriers where the big path has kernel boundaries.  49 us for BASELINE configs[3]'s 1 024
//  streams against 11 launches x 4.5 us: what a small launch costs is its own chain of dependent memory accesses --
//  find_stream's binary search, the size chain, the neighbours' records -- not the launch, and one workgroup walks
//  those chains eight deep where the grid walks them side by side.  profiles/r03_c4_timeline.txt.)
constexpr uint64_t SMALL_INPUT_BYTES = 4096u * 1024u;

// the index's kernels, in order, on `st`
static void enqueue_index(dvda_mlp_hip_ctx *c, hipStream_t st, const uint8_t *d_bytes, uint64_t total_bytes,
                          const uint64_t *d_stream_off, const uint64_t *d_stream_len, uint32_t n_streams)
{
    const uint64_t tiles = c->tiles;
    const uint32_t ms = c->max_segments;
    {
        uint32_t n_init = n_streams > ms ? n_streams : ms;
        if (n_init < 1024)
            n_init = 1024;              // (the summary's 520 words are zeroed by this grid too)
        hipLaunchKernelGGL(k_init_streams, dim3((n_init + 255) / 256), dim3(256), 0, st, c->d_streams,
                           n_streams, c->d_seg_status, c->d_seg_rows, c->d_yield, c->d_seg_meta, ms, c->d_cls,
                           reinterpret_cast<uint32_t *>(c->d_summary.p));
        hipLaunchKernelGGL(k_check_ranges, dim3(1), dim3(1024), 0, st, d_stream_off, d_stream_len, n_streams, total_bytes,
                           c->d_soff, c->d_slen, c->d_streams);
        d_stream_off = c->d_soff;
        d_stream_len = c->d_slen;
    }
    hipLaunchKernelGGL(k_sync_mask, dim3((unsigned)tiles), dim3(IDX_THREADS), 0, st, d_bytes,
                       total_bytes, c->d_masks, c->d_tile_count, c->d_parts);
    enqueue_exscan(st, c->d_tile_count, c->d_tile_base, c->d_scan_tmp, (uint32_t)tiles, nullptr, (uint32_t)tiles);
    hipLaunchKernelGGL(k_sync_scatter, dim3((unsigned)tiles), dim3(IDX_THREADS), 0, st, c->d_masks,
                       total_bytes, c->d_tile_base, c->d_cand_off, ms);
    hipLaunchKernelGGL(k_chase, dim3((ms + 255) / 256), dim3(256), 0, st, d_bytes, d_stream_off,
                       d_stream_len, n_streams, c->d_cand_off, c->d_n_cand, ms, c->d_seg,
                       c->d_seg_frames, c->d_streams, c->d_cls);
    hipLaunchKernelGGL(k_mark_dead, dim3((ms + 255) / 256), dim3(256), 0, st, d_stream_off, d_stream_len,
                       c->d_n_cand, ms, c->d_seg, c->d_seg_frames, c->d_streams);
    enqueue_exscan(st, c->d_seg_frames, c->d_seg_fbase, c->d_scan_tmp, 0u, c->d_n_cand, ms);
    // (a small input is decoded by the cooperative kernel, which has a workgroup per segment and no use for the lane
    //  packing: its four launches -- 18 us of early exits on a batch of one shape -- are left out, and k_link notes
    //  "mixes shapes" where no kernel looks, so that the lane kernels, should a caller force them, keep index order)
    const bool pack = !(total_bytes <= SMALL_INPUT_BYTES);
    hipLaunchKernelGGL(k_link, dim3((ms + 255) / 256), dim3(256), 0, st, d_stream_off, d_stream_len,
                       c->d_n_cand, ms, c->d_seg, c->d_seg_fbase, c->d_streams, n_streams, c->d_shape_key,
                       c->d_cls + (pack ? 2 : 3));
    // lane packing by stream shape (identity, and next to free, when the batch has one shape) -- five or six small
    // launches that nothing but the decode waits for: on a side stream, beside k_au_check (round 5: 25 us of the
    // bench batch's index, 0.2 ms of a batch of 16 384 streams of mixed shapes).  Forked and joined by events, which a
    // stream capture turns into the graph's edges.
    hipStream_t sp = st;
    bool forked = false;
    if (pack && st != nullptr && c->st_aux && hipEventRecord(c->ev_fork, st) == hipSuccess &&
        hipStreamWaitEvent(c->st_aux, c->ev_fork, 0) == hipSuccess) {
        sp = c->st_aux;
        forked = true;
    }
    if (pack) {
    hipLaunchKernelGGL(k_stream_rank, dim3((n_streams + 255) / 256), dim3(256), 0, sp, c->d_shape_key, c->d_streams,
                       n_streams, c->d_rank, c->d_sorted_cnt, c->d_cls + 2);
    enqueue_exscan(sp, c->d_sorted_cnt, c->d_sorted_base, c->d_scan_tmp, n_streams, nullptr, n_streams);
    (void)hipMemsetAsync(c->d_lane_seg, 0xFF, (size_t)ms * sizeof(uint32_t), sp);     // lanes that are dealt nothing
    hipLaunchKernelGGL(k_lane_perm, dim3((ms + 255) / 256), dim3(256), 0, sp, c->d_seg, c->d_streams, c->d_n_cand, ms,
                       c->d_rank, c->d_sorted_base, c->d_cls + 2, c->d_lane_seg);
    }
    // parity / CRC-8 of every substream, byte-parallel (8 lanes per segment): the decode lanes only compare
    hipLaunchKernelGGL(k_au_check, dim3((unsigned)(((uint64_t)ms * CHK_GROUP + CHK_THREADS - 1) / CHK_THREADS)),
                       dim3(CHK_THREADS), 0, st, d_bytes, c->d_parts, c->d_seg, c->d_n_cand, ms, c->d_streams, c->d_seg_check);
    if (forked) {
        (void)hipEventRecord(c->ev_join, sp);
        (void)hipStreamWaitEvent(st, c->ev_join, 0);
    }
}

static int index_source(dvda_mlp_hip_ctx *c, const uint8_t *d_bytes, uint64_t total_bytes,
                        const uint64_t *d_stream_off, const uint64_t *d_stream_len, uint32_t n_streams, void *stream_)
{
    if (!c || !d_bytes || !d_stream_off || !d_stream_len || n_streams == 0 || total_bytes == 0)
        return DVDA_HIP_EINVAL;
    if (n_streams > c->max_streams)
        return DVDA_HIP_ECAPACITY;
    if (((uintptr_t)d_bytes & 15) != 0)
        return DVDA_HIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    c->cc.spans.clear();
    c->cc.info.clear();
    int rc = ensure_byte_ws(c, total_bytes);
    if (rc)
        return rc;
    c->d_bytes = d_bytes;
    c->total_bytes = total_bytes;
    c->d_stream_off = d_stream_off;
    c->d_stream_len = d_stream_len;
    c->n_streams = n_streams;
    const uint64_t chunks = (total_bytes + 15) / 16;
    const uint64_t tiles = (chunks + IDX_TILE_CHUNKS - 1) / IDX_TILE_CHUNKS;
    c->tiles = tiles;
    c->d_n_cand = c->d_tile_base + tiles;

    c->small_input = total_bytes <= SMALL_INPUT_BYTES;
    // The launch sequence depends on the call's arguments only.  A caller that indexes the same buffers again
    // (third call on: seen, captured, replayed) gets it as ONE graph launch; capture needs a real stream (not
    // the legacy default stream), anything going wrong with it switches the graph off for this context.
    const bool same = c->idx_graph_state > 0 && c->idx_key[0] == d_bytes && c->idx_key[1] == d_stream_off &&
                      c->idx_key[2] == d_stream_len && c->idx_key[3] == (const void *)st &&
                      c->idx_key_bytes == total_bytes && c->idx_key_streams == n_streams;
    if (c->idx_graph_state == 2 && same) {
        if (hipGraphLaunch(c->idx_graph, st) == hipSuccess) {
            c->indexed = true;
            c->decoded = false;
            return DVDA_HIP_OK;
        }
        (void)hipGetLastError();
        c->idx_graph_state = -1;
    } else if (c->idx_graph_state == 1 && same && st != nullptr) {
        hipGraph_t g = nullptr;
        bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            enqueue_index(c, st, d_bytes, total_bytes, d_stream_off, d_stream_len, n_streams);
            ok = hipStreamEndCapture(st, &g) == hipSuccess && g != nullptr;
        }
        if (ok) {
            ok = hipGraphInstantiate(c->idx_graph.put(), g, nullptr, nullptr, 0) == hipSuccess;
        }
        if (g)
            (void)hipGraphDestroy(g);
        if (ok && hipGraphLaunch(c->idx_graph, st) == hipSuccess) {
            c->idx_graph_state = 2;
            c->indexed = true;
            c->decoded = false;
            return DVDA_HIP_OK;
        }
        (void)hipGetLastError();
        c->idx_graph_state = -1;                 // direct launches from here on
    } else if (c->idx_graph_state >= 0) {
        c->idx_key[0] = d_bytes;
        c->idx_key[1] = d_stream_off;
        c->idx_key[2] = d_stream_len;
        c->idx_key[3] = (const void *)st;
        c->idx_key_bytes = total_bytes;
        c->idx_key_streams = n_streams;
        c->idx_graph_state = 1;
    }
    enqueue_index(c, st, d_bytes, total_bytes, d_stream_off, d_stream_len, n_streams);
    HIP_TRY(hipGetLastError());
    c->indexed = true;
    c->decoded = false;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_index(dvda_mlp_hip_ctx *c, const uint8_t *d_bytes, uint64_t total_bytes,
                                  const uint64_t *d_stream_off, const uint64_t *d_stream_len,
                                  uint32_t n_streams, void *stream_)
{
    const int rc = index_source(c, d_bytes, total_bytes, d_stream_off, d_stream_len, n_streams, stream_);
    if (rc != DVDA_HIP_OK || c->pp.mode != DVDA_PRESENT_SUBSTREAM0)
        return rc;
    // presentation: the source's index is there; strip, and index what is left (mlp_present_run.h)
    return present_index(c, (hipStream_t)stream_);
}

static int read_summary(dvda_mlp_hip_ctx *c, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(DecodeSummary), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DVDA_HIP_OK;
}

// The chain passes' workspaces hold less than the plan asks for (a non-blocking decode runs on what
// dvda_mlp_hip_reserve left): nothing is deferred to them then -- the plan's totals are zeroed, every chain kernel
// behind this one finds no work, and the segments that waited are reported DVDA_ST_CAPACITY by the last k_finalize.
__global__ void k_chain_guard(uint4 *plan, const uint32_t *n_seg_ptr, uint32_t max_seg, WsCaps caps, uint32_t seg_cap)
{
    uint32_t n = *n_seg_ptr;
    if (n > max_seg)
        n = max_seg;
    const uint4 t = plan[n];
    const unsigned long long rows = t.x, segs = t.y;
    const ChainNeed need = chain_need(rows, segs);
    if (segs > seg_cap || need.res > caps.res || need.brec > caps.brec || need.frec > caps.frec)
        plan[n] = make_uint4(t.x, 0, 0, 0);
}

// the chain passes' workspaces for `segs` deferred segments of `rows` PCM frames (mlp_bounds.h: chain_need)
static int grow_chain_ws(dvda_mlp_hip_ctx *c, uint64_t rows, uint64_t segs)
{
    const ChainNeed need = chain_need(rows, segs);
    int rc;
    if ((rc = c->d_res.grow(need.res)) != 0 || (rc = c->d_brec.grow(need.brec)) != 0)
        return rc;
    return c->d_frec.grow(need.frec);
}

// the sequential pass's frame buffers: one per stream of a round
static int grow_fb(dvda_mlp_hip_ctx *c, uint32_t round)
{
    return c->d_fb.grow_exact((uint64_t)round * FB_WORDS);
}

// presentation: a call that decodes (or reserves for a decode) is the inner context's, with the settings the caller
// gave this one -- the one place they are handed on (they are read by the decode passes only, never by the index)
static dvda_mlp_hip_ctx *pp_forward(dvda_mlp_hip_ctx *c)
{
    dvda_mlp_hip_ctx *x = pp_inner(c);
    if (x)
        x->set = c->set;
    return x;
}

extern "C" int dvda_mlp_hip_reserve(dvda_mlp_hip_ctx *c, uint64_t chain_pcm_frames, uint32_t chain_segments,
                                    uint32_t seq_streams)
{
    if (!c)
        return DVDA_HIP_EINVAL;
    if (dvda_mlp_hip_ctx *x = pp_forward(c))
        return dvda_mlp_hip_reserve(x, chain_pcm_frames, chain_segments, seq_streams);
    HIP_TRY(hipSetDevice(c->device));
    if (chain_pcm_frames >> 32)
        return DVDA_HIP_ECAPACITY;
    if (chain_segments || chain_pcm_frames) {
        const int rc = grow_chain_ws(c, chain_pcm_frames, chain_segments);
        if (rc)
            return rc;
        if (chain_segments > c->rsv_segs)
            c->rsv_segs = chain_segments;
    }
    return grow_fb(c, seq_streams < SEQ_ROUND ? seq_streams : SEQ_ROUND);
}

// which fast-pass kernels a decode call launches, from the caller's lane setting and the size of the input: one lane
// per segment either way -- the one-substream kernel and the one whose lane reads both substreams of its segment
// (DUO) -- both unless the caller forced the first; a kernel whose class is absent from the batch (the index knows)
// exits at once
// (64: always the wave-cooperative kernel; 0: the device picks it for small batches -- coop_takes() -- and the
//  lane kernels for everything else; 1 / 2 force a lane kernel)
// (3: the lane kernels, picked per batch as under 0, but never the cooperative kernel)
// (a small input is the cooperative kernel's whatever it holds: SMALL_INPUT_BYTES)
struct KernelChoice {
    bool coop_only, lanes_only;
    uint32_t force;         // 0, or the lane kernel the caller forced (1 / 2)

    explicit KernelChoice(const dvda_mlp_hip_ctx *c)
        : coop_only(c->set.lanes_per_seg == 64 || (c->set.lanes_per_seg == 0 && c->small_input)),
          lanes_only(c->set.lanes_per_seg == 3), force((coop_only || lanes_only) ? 0u : c->set.lanes_per_seg)
    {
    }
};

// What the passes behind the fast pass work on.  A blocking call reads it from the summary the pass before left; a
// non-blocking call (dvda_mlp_hip_decode_async) reads nothing back: it goes by what dvda_mlp_hip_reserve left, and the
// kernels find their work -- or none -- on the device.  Taken at the top of each pass.
struct PassWork {
    uint32_t segs;          // deferred segments
    uint64_t rows;          // their PCM frames at the standard timing (non-blocking: 0, the workspaces are not sized here)
    uint32_t max_rows;      // the longest of them (non-blocking: 0)
    // few chains: the lean two-pass form.  (How many CHAINS there are is what decides -- a chain is serial, and the
    // fused kernel's pace per chain is a third of the lean filter's -- and chains are at most a few per stream: the
    // streams that wait for these passes, counted by k_finalize, stand in for them; the non-blocking call goes by
    // its reservation)
    bool few;
    uint32_t n_seq;         // streams of the sequential pass (non-blocking: the frame buffers reserved)
};
static PassWork pass_work(const dvda_mlp_hip_ctx *c, bool blocking)
{
    const DecodeSummary &s = *c->h_summary;
    if (blocking)
        return {s.chain_segs, s.chain_rows, s.chain_max_rows, s.waiting <= CHAIN_SMALL_STREAMS, s.seq_streams};
    return {c->rsv_segs, 0, 0, c->rsv_segs <= CHAIN_SMALL_SEGS, c->fb_slots()};
}

static DecodeArgs decode_args(const dvda_mlp_hip_ctx *c, const KernelChoice &k, int32_t *d_pcm, const uint64_t *d_out_off,
                              const uint64_t *d_out_stride)
{
    DecodeArgs a;
    memset(&a, 0, sizeof(a));
    a.bytes = c->d_bytes;
    a.total_bytes = c->total_bytes;
    a.seg = c->d_seg;
    a.seg_fbase = c->d_seg_fbase;
    a.n_seg_ptr = c->d_n_cand;
    a.max_seg = c->max_segments;
    a.streams = c->d_streams;
    a.pcm = d_pcm;
    a.out_off = d_out_off;
    a.out_stride = d_out_stride;
    a.seg_status = c->d_seg_status;
    a.seg_rows = c->d_seg_rows;
    a.iir_ws = c->d_iir;
    a.mat_ws = c->d_mat;
    a.total_lanes = c->iir_lanes;
    a.dbg = c->d_dbg;
    a.fir_ws = c->d_fir;
    a.init_fir = c->set.d_init_fir;
    a.summary = c->d_summary;
    a.interleaved = c->set.pcm_layout != DVDA_PCM_PLANAR;
    a.wav_bits = c->set.pcm_layout == DVDA_PCM_WAV24 ? 24u : c->set.pcm_layout == DVDA_PCM_WAV16 ? 16u : 0u;
    a.coop_min_seg = c->coop_min_seg;
    a.cls = c->d_cls;
    a.hetero = c->d_cls + 2;
    a.lane_seg = c->d_lane_seg;
    a.seg_meta = c->d_seg_meta;
    a.yield_req = c->d_yield;
    a.seg_check = c->d_seg_check;
    a.caps = ws_caps(c);
    a.coop = k.coop_only ? 64u : k.lanes_only ? 3u : k.force;
    return a;
}

// (after the chain workspaces have their size for this call)
static ChainArgs chain_args(const dvda_mlp_hip_ctx *c, const DecodeArgs &a)
{
    ChainArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.caps = a.caps;
    ca.seg = c->d_seg;
    ca.seg_fbase = c->d_seg_fbase;
    ca.n_seg_ptr = c->d_n_cand;
    ca.max_seg = c->max_segments;
    ca.streams = c->d_streams;
    ca.seg_status = c->d_seg_status;
    ca.seg_rows = c->d_seg_rows;
    ca.seg_meta = c->d_seg_meta;
    ca.plan = c->d_plan;
    ca.def_list = c->d_def_list;
    ca.head_list = c->d_head_list;
    ca.chain_order = c->d_chain_order;
    ca.chain_hist = c->d_chain_hist;
    ca.res = c->d_res;
    ca.brec = c->d_brec;
    ca.frec = c->d_frec;
    ca.fir_ws = c->d_fir;
    ca.total_lanes = c->iir_lanes;
    ca.init_fir = c->set.d_init_fir;
    ca.pcm = a.pcm;
    ca.out_off = a.out_off;
    ca.out_stride = a.out_stride;
    ca.interleaved = a.interleaved;
    ca.wav_bits = a.wav_bits;
    ca.dbg = c->d_dbg;
    return ca;
}

// k_finalize: the segments' findings folded into their streams -- behind the fast pass and the chain passes (what still
// waits is counted and listed for the pass behind), and `last`: the final word on every stream
static void enqueue_finalize(dvda_mlp_hip_ctx *c, hipStream_t st, bool last)
{
    const dim3 fgrid((unsigned)(((uint64_t)c->n_streams * FIN_GROUP + 255) / 256));
    hipLaunchKernelGGL(k_finalize, fgrid, dim3(256), 0, st, c->d_seg, c->d_seg_fbase, c->d_seg_status, c->d_seg_rows,
                       c->d_streams, c->n_streams, c->d_summary, c->d_seq_list, last ? 0u : 1u, last ? 1u : 0u,
                       c->d_seg_check);
}

// ---- fast pass: every segment, a lane (or a workgroup of the cooperative kernel) each
static void fast_pass(dvda_mlp_hip_ctx *c, hipStream_t st, const KernelChoice &k, DecodeArgs &a)
{
    const uint64_t ms = c->max_segments;
    const unsigned blocks1 = (unsigned)((ms + DEC_THREADS - 1) / DEC_THREADS);            // one lane per segment
    // (1: the one-substream lane kernel for every stream -- a two-substream stream is then an envelope error; 2 and 3: both
    //  lane kernels, each on its class of streams -- the two-substream kernel decodes two-substream streams only)
    const bool run1 = !k.coop_only, run2 = k.force != 1 && !k.coop_only;
    if (k.coop_only || (k.force == 0 && !k.lanes_only)) {
        const unsigned cblocks = (unsigned)(k.coop_only || ms < COOP_MAX_SEG ? ms : COOP_MAX_SEG);
        hipLaunchKernelGGL(k_coop<false>, dim3(cblocks), dim3(COOP_THREADS), 0, st, a);
    }
    if (run1) {
        a.only_S = (k.force == 1) ? 0u : 1u;
        if (a.interleaved && a.wav_bits)
            hipLaunchKernelGGL((k_decode<6, false, false, true, false, false, true>), dim3(blocks1), dim3(DEC_THREADS), 0, st, a);
        else if (a.interleaved)
            hipLaunchKernelGGL((k_decode<6, false, false, true>), dim3(blocks1), dim3(DEC_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL((k_decode<6, false, false>), dim3(blocks1), dim3(DEC_THREADS), 0, st, a);
    }
    if (run2) {
        // two-substream streams: one lane reads both substreams of its segment (k_decode<.., DUO>)
        a.only_S = 2u;
        if (a.interleaved)
            hipLaunchKernelGGL((k_decode<6, false, false, true, false, true>), dim3(blocks1), dim3(DEC_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL((k_decode<6, false, false, false, false, true>), dim3(blocks1), dim3(DEC_THREADS), 0, st, a);
    }
}

// ---- chain passes: segments that continue the FIR history of the one before them, or change
//      matrix-class parameters inside an access unit
static int chain_passes(dvda_mlp_hip_ctx *c, hipStream_t st, const KernelChoice &k, DecodeArgs &a, bool blocking)
{
    const PassWork w = pass_work(c, blocking);
    if (w.segs == 0)
        return DVDA_HIP_OK;
    const uint32_t segs = w.segs;
    const uint64_t ms = c->max_segments;
    int rc;
    if (w.rows >> 32)
        return DVDA_HIP_ECAPACITY;          // plan entries are 32-bit (137 GB of planes)
    if (blocking && (rc = grow_chain_ws(c, w.rows, segs)) != 0)
        return rc;
    a.caps = ws_caps(c);
    ChainArgs ca = chain_args(c, a);
    const unsigned sblocks = (unsigned)((ms + 1023) / 1024);
    hipLaunchKernelGGL(k_chain_plan, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(k_scan4_blocks, dim3(sblocks), dim3(1024), 0, st, c->d_plan, c->d_scan4_tmp, c->d_n_cand,
                       c->max_segments);
    hipLaunchKernelGGL(k_scan4_sums, dim3(1), dim3(1024), 0, st, c->d_scan4_tmp, sblocks);
    hipLaunchKernelGGL(k_scan4_add, dim3(sblocks), dim3(1024), 0, st, c->d_plan, c->d_scan4_tmp, sblocks,
                       c->d_n_cand, c->max_segments);
    if (!blocking)
        hipLaunchKernelGGL(k_chain_guard, dim3(1), dim3(1), 0, st, c->d_plan, c->d_n_cand, c->max_segments, a.caps, segs);
    hipLaunchKernelGGL(k_chain_lists, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, ca);
    // parse: lane (pair) j takes deferred segment def_list[j]
    a.list = c->d_def_list;
    a.list_base = 0;
    a.list_n = segs;
    a.plan = c->d_plan;
    a.res = c->d_res;
    a.brec = c->d_brec;
    a.frec = c->d_frec;
    // (few deferred segments -- one chained title, a small batch: a workgroup per segment, mlp_coop.h; a lane of
    //  k_decode needs 1.6 ms for a segment of eight units however few there are.  Known on the host in the
    //  blocking call; the non-blocking one sizes by its reservation.)
    const bool coop_parse = k.coop_only || (c->set.lanes_per_seg == 0 && segs <= COOP_MAX_SEG);
    if (coop_parse) {
        hipLaunchKernelGGL(k_coop<true>, dim3(segs), dim3(COOP_THREADS), 0, st, a);
    } else {
        a.only_S = (k.force == 1) ? 0u : 1u;
        hipLaunchKernelGGL((k_decode<6, false, false, false, true>), dim3((segs + DEC_THREADS - 1) / DEC_THREADS),
                           dim3(DEC_THREADS), 0, st, a);
        if (k.force != 1) {
            a.only_S = 2u;
            hipLaunchKernelGGL((k_decode<6, false, false, false, true, true>), dim3((segs + DEC_THREADS - 1) / DEC_THREADS),
                               dim3(DEC_THREADS), 0, st, a);
        }
    }
    if (c->set.chain_form == 2 || (c->set.chain_form == 0 && w.few)) {
        // few chains (one title, a small batch): the lean two-pass form (mlp_chain_small.h)
        // filter: 16 lanes per chain (at most one chain per deferred segment)
        hipLaunchKernelGGL(k_chain_filter, dim3((unsigned)(((uint64_t)segs * 16 + 63) / 64)), dim3(64), 0, st, ca);
        // rematrix: one lane per PCM frame (a workgroup walks its segment 256 PCM frames at a time; segments of more
        // than 16 such blocks share the walk between several workgroups)
        ca.remat_blocks = (w.max_rows + 4095) / 4096 ? (w.max_rows + 4095) / 4096 : 1;
        hipLaunchKernelGGL(k_chain_rematrix, dim3(segs * ca.remat_blocks), dim3(256), 0, st, ca);
    } else {
        // the chains longest first (k_chain_fused's workgroups take eight neighbours of that order)
        HIP_TRY(hipMemsetAsync(c->d_chain_hist, 0, CHAIN_BUCKETS * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_chain_hist, dim3((segs + 255) / 256), dim3(256), 0, st, ca);
        hipLaunchKernelGGL(k_chain_scan, dim3(1), dim3(CHAIN_BUCKETS), 0, st, ca);
        hipLaunchKernelGGL(k_chain_scatter, dim3((segs + 255) / 256), dim3(256), 0, st, ca);
        // filter + rematrix in one walk over the planes: two waves per eight chains (at most one chain per deferred segment)
        hipLaunchKernelGGL(k_chain_fused, dim3((unsigned)(((uint64_t)segs + 7) / 8)), dim3(FU_THREADS), 0, st, ca);
    }
    HIP_TRY(hipMemsetAsync(&c->d_summary->seq_streams, 0, sizeof(uint32_t), st));
    enqueue_finalize(c, st, false);
    HIP_TRY(hipGetLastError());
    return blocking ? read_summary(c, st) : DVDA_HIP_OK;
}

// ---- sequential pass: streams with non-standard timing, IIR taps or restart headers inside an access
//      unit, whole and in order, one lane pair and one frame buffer per stream, a round at a time
// -> *ran: the pass had streams to decode
static int sequential_pass(dvda_mlp_hip_ctx *c, hipStream_t st, DecodeArgs &a, bool blocking, bool *ran)
{
    const uint32_t n_seq = pass_work(c, blocking).n_seq;
    *ran = n_seq != 0;
    if (!n_seq)
        return DVDA_HIP_OK;
    const uint32_t round = n_seq < SEQ_ROUND ? n_seq : SEQ_ROUND;
    int rc;
    if (blocking && (rc = grow_fb(c, round)) != 0)
        return rc;
    a.fb = c->d_fb;
    a.caps = ws_caps(c);
    a.list = c->d_seq_list;
    a.only_S = 0;
    // (non-blocking: ONE round of as many streams as frame buffers were reserved; how many streams there are
    //  the kernel reads on the device, and what does not fit is reported by the last k_finalize)
    a.list_n_ptr = blocking ? nullptr : &c->d_summary->seq_streams;
    for (uint32_t base = 0; base < n_seq; base += round) {
        a.list_base = base;
        a.list_n = n_seq - base < round ? n_seq - base : round;
        hipLaunchKernelGGL((k_decode<6, true, true>), dim3((2 * a.list_n + DEC_THREADS - 1) / DEC_THREADS),
                           dim3(DEC_THREADS), 0, st, a);
    }
    return DVDA_HIP_OK;
}

static int decode_body(dvda_mlp_hip_ctx *c, int32_t *d_pcm, const uint64_t *d_out_off, const uint64_t *d_out_stride,
                       void *stream_, bool blocking, bool *counted, uint32_t *slot_out)
{
    if (!c || !d_pcm || !d_out_off || !d_out_stride)
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const KernelChoice k(c);
    DecodeArgs a = decode_args(c, k, d_pcm, d_out_off, d_out_stride);
    if (c->decoded) {               // (the first decode on an index finds the summary zeroed by the index)
        HIP_TRY(hipMemsetAsync(c->d_summary, 0, (1 + SUMMARY_PARTS) * sizeof(DecodeSummary), st));
        hipLaunchKernelGGL(k_reset_segments, dim3((unsigned)((c->max_segments + 255) / 256)), dim3(256), 0, st,
                           c->d_seg_status, c->d_seg_rows, c->d_yield, c->d_seg_meta, c->max_segments);
    }
    c->decoded = true;

    // (timed: the dominant kernel)
    const uint32_t slot = (uint32_t)(c->ev_count % EV_RING);
    HIP_TRY(hipEventRecord(c->ev[2 * slot], st));
    fast_pass(c, st, k, a);
    HIP_TRY(hipEventRecord(c->ev[2 * slot + 1], st));
    c->ev_count++;
    *counted = true;
    *slot_out = slot;
    enqueue_finalize(c, st, false);
    HIP_TRY(hipGetLastError());
    // A blocking call waits for the fast pass here: its summary says what else is launched and how large the chain
    // workspaces have to be.  A non-blocking call (dvda_mlp_hip_decode_async) never waits and never allocates: the
    // passes behind the fast pass are enqueued on the workspaces dvda_mlp_hip_reserve left, sized for what was
    // reserved, and find their work -- or none -- on the device.
    int rc = 0;
    if (blocking && (rc = read_summary(c, st)) != 0)
        return rc;
    if ((rc = chain_passes(c, st, k, a, blocking)) != 0)
        return rc;
    bool seq_ran = false;
    if ((rc = sequential_pass(c, st, a, blocking, &seq_ran)) != 0)
        return rc;
    // (`waiting` without either: the lanes' count of deferred segments and the segments' status disagree -- the
    //  last finalize then reports what was left undecoded instead of passing it as clean)
    if (!blocking || c->h_summary->chain_segs || seq_ran || c->h_summary->waiting)
        enqueue_finalize(c, st, true);
    HIP_TRY(hipEventRecord(c->ev_end[slot], st));
    HIP_TRY(hipGetLastError());
    return DVDA_HIP_OK;
}

static int decode_impl(dvda_mlp_hip_ctx *c, int32_t *d_pcm, const uint64_t *d_out_off, const uint64_t *d_out_stride,
                       void *stream_, bool blocking)
{
    // (a call that was counted in the event ring has its end event recorded whichever way it leaves: the timing call
    //  measures start -> end of every counted call)
    bool counted = false;
    uint32_t slot = 0;
    const int rc = decode_body(c, d_pcm, d_out_off, d_out_stride, stream_, blocking, &counted, &slot);
    if (counted && rc != DVDA_HIP_OK)
        (void)hipEventRecord(c->ev_end[slot], (hipStream_t)stream_);
    return rc;
}

extern "C" int dvda_mlp_hip_decode(dvda_mlp_hip_ctx *c, int32_t *d_pcm, const uint64_t *d_out_off,
                                   const uint64_t *d_out_stride, void *stream_)
{
    if (dvda_mlp_hip_ctx *x = pp_forward(c))
        return c->indexed ? dvda_mlp_hip_decode(x, d_pcm, d_out_off, d_out_stride, stream_) : DVDA_HIP_ESTATE;
    if (c) {
        c->cc.spans.clear();
        c->cc.info.clear();
        c->cc.ran = false;
    }
    const int rc = decode_impl(c, d_pcm, d_out_off, d_out_stride, stream_, true);
    if (rc != DVDA_HIP_OK || !c->cc.on)
        return rc;
    return conceal_run(c, d_pcm, d_out_off, d_out_stride, (hipStream_t)stream_);
}

extern "C" int dvda_mlp_hip_decode_async(dvda_mlp_hip_ctx *c, int32_t *d_pcm, const uint64_t *d_out_off,
                                         const uint64_t *d_out_stride, void *stream_)
{
    if (dvda_mlp_hip_ctx *x = pp_forward(c))
        return c->indexed ? dvda_mlp_hip_decode_async(x, d_pcm, d_out_off, d_out_stride, stream_) : DVDA_HIP_ESTATE;
    if (c && c->cc.on)
        return DVDA_HIP_EINVAL;     // concealing reads the damage back: the blocking call only
    return decode_impl(c, d_pcm, d_out_off, d_out_stride, stream_, false);
}

extern "C" int dvda_mlp_hip_set_pcm_layout(dvda_mlp_hip_ctx *c, uint32_t layout)
{
    if (!c || layout > DVDA_PCM_WAV16)
        return DVDA_HIP_EINVAL;
    c->set.pcm_layout = layout;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_set_chain_form(dvda_mlp_hip_ctx *c, uint32_t form)
{
    if (!c || form > 2)
        return DVDA_HIP_EINVAL;
    c->set.chain_form = form;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_set_lanes_per_segment(dvda_mlp_hip_ctx *c, uint32_t lanes)
{
    if (!c || (lanes > 3 && lanes != 64))
        return DVDA_HIP_EINVAL;
    c->set.lanes_per_seg = lanes;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_stream_info(dvda_mlp_hip_ctx *c, dvda_mlp_stream_info *infos, uint32_t n,
                                        void *stream_)
{
    if (!c || !infos)
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    if (pp_inner(c))
        return present_stream_info(c, infos, n, stream_);
    if (n > c->n_streams)
        n = c->n_streams;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    std::vector<StreamRec> h(n);
    HIP_TRY(hipMemcpy(h.data(), c->d_streams, (size_t)n * sizeof(StreamRec), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        dvda_mlp_stream_info &o = infos[i];
        memset(&o, 0, sizeof(o));
        o.mlp_frames = h[i].frames;
        o.pcm_frames = h[i].rows;
        o.bytes_consumed = h[i].consumed;
        o.status = h[i].status;
        fill_sync_fields(o, h[i].sync);
        o.channels = channel_count(o.assignment);
        o.segments = h[i].n_seg;
        if (i < c->cc.info.size() && c->cc.info[i].valid) {
            // conceal mode: the stream as it was handed out (kept + silence + resumed)
            o.status = c->cc.info[i].status;
            o.pcm_frames = c->cc.info[i].rows;
            o.mlp_frames = c->cc.info[i].frames;
        }
    }
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_segment_count(dvda_mlp_hip_ctx *c, uint32_t *n_segments, void *stream_)
{
    if (!c || !n_segments)
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    HIP_TRY(hipMemcpy(n_segments, c->d_n_cand, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (*n_segments > c->max_segments)
        return DVDA_HIP_ECAPACITY;
    // (presentation: a source with more major syncs than the context holds was indexed in part -- the caller's cue to
    //  come back with a larger context, as without the presentation; else the count is the inner context's)
    dvda_mlp_hip_ctx *x = pp_inner(c);
    return x ? dvda_mlp_hip_segment_count(x, n_segments, stream_) : DVDA_HIP_OK;
}

// how the last index call's launches went out (idx_graph_state, mlp_ctx.h): tests read it to know the replay ran
extern "C" int dvda_mlp_hip_index_graph_state(dvda_mlp_hip_ctx *c, int *state)
{
    if (!c || !state)
        return DVDA_HIP_EINVAL;
    *state = c->idx_graph_state;
    return DVDA_HIP_OK;
}

// mean device ms of the newest decode calls in the event ring, each from its first kernel to the event end_of(slot)
template <typename EndOf>
static int ring_mean(dvda_mlp_hip_ctx *c, EndOf end_of, double *avg_ms, uint32_t *count)
{
    HIP_TRY(hipSetDevice(c->device));
    double total = 0;
    // the ring holds the newest EV_RING decode calls
    const uint32_t n = c->ev_count < EV_RING ? (uint32_t)c->ev_count : EV_RING;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t slot = (uint32_t)((c->ev_count - 1 - i) % EV_RING);
        const hipEvent_t end = end_of(slot);
        HIP_TRY(hipEventSynchronize(end));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[2 * slot], end));
        total += ms;
    }
    *avg_ms = n ? total / n : 0.0;
    if (count)
        *count = n;
    return DVDA_HIP_OK;
}

// the fast pass alone; resets the ring
extern "C" int dvda_mlp_hip_kernel_time(dvda_mlp_hip_ctx *c, double *avg_ms, uint32_t *launches)
{
    if (!c || !avg_ms)
        return DVDA_HIP_EINVAL;
    if (dvda_mlp_hip_ctx *x = pp_inner(c))
        return dvda_mlp_hip_kernel_time(x, avg_ms, launches);
    const int rc = ring_mean(c, [c](uint32_t slot) -> hipEvent_t { return c->ev[2 * slot + 1]; }, avg_ms, launches);
    if (rc == DVDA_HIP_OK)
        c->ev_count = 0;
    return rc;
}

// the same ring, first kernel of a decode call to its last (fast pass + whatever ran behind it, and the gaps in
// between): does not reset the ring -- call it BEFORE dvda_mlp_hip_kernel_time
extern "C" int dvda_mlp_hip_decode_time(dvda_mlp_hip_ctx *c, double *avg_ms, uint32_t *calls)
{
    if (!c || !avg_ms)
        return DVDA_HIP_EINVAL;
    if (dvda_mlp_hip_ctx *x = pp_inner(c))
        return dvda_mlp_hip_decode_time(x, avg_ms, calls);
    return ring_mean(c, [c](uint32_t slot) -> hipEvent_t { return c->ev_end[slot]; }, avg_ms, calls);
}

// diagnostic builds (DVDA_EXP_STAMP): reads and clears 16 of the per-phase cycle sums
static int debug_counters(dvda_mlp_hip_ctx *c, uint32_t first, unsigned long long *out16)
{
    if (!c || !out16)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, c->d_dbg + first, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(c->d_dbg + first, 0, 16 * sizeof(unsigned long long)));
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_debug_counters(dvda_mlp_hip_ctx *c, unsigned long long *out16) { return debug_counters(c, 0, out16); }

// ... and the second half of them: k_chain_fused's two waves (tools/probe/fused_stamp.py)
extern "C" int dvda_mlp_hip_debug_counters2(dvda_mlp_hip_ctx *c, unsigned long long *out16) { return debug_counters(c, 16, out16); }

// host_out[book * 512 + peek9] = value | length << 8 as the row loop's arithmetic code-book decode sees it
extern "C" int dvda_mlp_hip_selftest_huff(int device, uint32_t *host_out)
{
    if (!host_out)
        return DVDA_HIP_EINVAL;
    uint32_t *d = nullptr;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc((void **)&d, 4 * 512 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_selftest_huff, dim3(8), dim3(256), 0, 0, d);
    const hipError_t e = hipMemcpy(host_out, d, 4 * 512 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? DVDA_HIP_OK : DVDA_HIP_ENODEV;
}

// host_out[i] = field i read from `bytes` by the kernels' bit reader (widths as in k_selftest_bits)
extern "C" int dvda_mlp_hip_selftest_bits(int device, const uint8_t *host_bytes, uint32_t n_bytes,
                                          const int32_t *host_widths, uint32_t n, int64_t *host_out, uint32_t resident)
{
    if (!host_bytes || !host_widths || !host_out || n == 0 || n_bytes == 0)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint8_t> d_b;
    DevBuf<int32_t> d_w;
    DevBuf<int64_t> d_o;
    const size_t padded = (((size_t)n_bytes + 63) & ~(size_t)63) + 128;
    hipError_t e = d_b.alloc(padded);
    if (e == hipSuccess)
        e = d_w.alloc(n);
    if (e == hipSuccess)
        e = d_o.alloc(n);
    if (e == hipSuccess)
        e = hipMemset(d_b, 0, padded);
    if (e == hipSuccess)
        e = hipMemcpy(d_b, host_bytes, n_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d_w, host_widths, n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_selftest_bits, dim3(1), dim3(64), 0, 0, d_b, n_bytes, d_w, n, d_o, resident);
        e = hipMemcpy(host_out, d_o, n * sizeof(int64_t), hipMemcpyDeviceToHost);
    }
    return e == hipSuccess ? DVDA_HIP_OK : DVDA_HIP_ENODEV;
}

extern "C" int dvda_mlp_hip_set_initial_fir(dvda_mlp_hip_ctx *c, const int32_t *d_init_fir)
{
    if (!c)
        return DVDA_HIP_EINVAL;
    c->set.d_init_fir = d_init_fir;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_segment_info(dvda_mlp_hip_ctx *c, uint32_t segment, dvda_mlp_segment_info *info,
                                         void *stream_)
{
    if (!c || !info)
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    if (pp_inner(c))
        return present_segment_info(c, segment, info, stream_);
    if (segment >= c->max_segments)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    SegRec r;
    uint32_t rows = 0, st = 0;
    HIP_TRY(hipMemcpy(&r, c->d_seg + segment, sizeof(r), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&rows, c->d_seg_rows + segment, sizeof(rows), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&st, c->d_seg_status + segment, sizeof(st), hipMemcpyDeviceToHost));
    info->offset = r.off;
    info->end = r.end;
    info->stream = r.stream;
    info->mlp_frames = r.nframes;
    info->pcm_frames = rows;
    info->status = st | r.flags;
    return DVDA_HIP_OK;
}

extern "C" int dvda_mlp_hip_segment_fir(dvda_mlp_hip_ctx *c, uint32_t segment, int32_t *host_fir, void *stream_)
{
    if (!c || !host_fir)
        return DVDA_HIP_EINVAL;
    if (!c->indexed)
        return DVDA_HIP_ESTATE;
    if (pp_inner(c))
        return dvda_mlp_hip_segment_fir(c->pp.child, segment, host_fir, stream_);
    const uint32_t L = 2;       // workspace lane = segment * 2 + substream in every pass
    if ((uint64_t)segment * L + L > c->iir_lanes)
        return DVDA_HIP_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    memset(host_fir, 0, 2 * 48 * sizeof(int32_t));
    for (uint32_t s = 0; s < L; s++) {
        // element (slot*8 + tap) of lane l lives at fir[(slot*8 + tap) * lanes + l]: a 48-row column
        HIP_TRY(hipMemcpy2D(host_fir + s * 48, sizeof(int32_t), c->d_fir + (size_t)segment * L + s,
                            (size_t)c->iir_lanes * sizeof(int32_t), sizeof(int32_t), 48,
                            hipMemcpyDeviceToHost));
    }
    return DVDA_HIP_OK;
}

