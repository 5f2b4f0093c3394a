// mlp_ctx.h -- host side of the batch tier: the context (every workspace a member that frees itself, hip_ws.h), the
// decode settings, the state of the two modes (conceal: mlp_conceal_run.h, presentation: mlp_present_run.h), and the
// scan launch every tier shares.
#pragma once
#include <vector>

#include "hip_ws.h"
#include "mlp_decode.h"
#include "mlp_conceal.h"
#include "mlp_index.h"

using namespace mlp;

constexpr uint32_t EV_RING = 256;       // decode calls whose kernel time is kept (the newest)
constexpr uint32_t SEQ_ROUND = 1024;    // streams one round of the sequential pass decodes

// What a decode call reads of the caller's choices -- and nothing but a decode call reads them (the index does not):
// a context that decodes for another one (the modes' children) is handed the whole record where the call is forwarded.
struct DecodeSettings {
    uint32_t lanes_per_seg = 0;             // 0: chosen per batch from the indexed substream counts
    uint32_t pcm_layout = DVDA_PCM_PLANAR;  // DVDA_PCM_*
    uint32_t chain_form = 0;                // 0: by the batch (few deferred segments: two passes, else the fused kernel); 1: fused; 2: two passes
    const int32_t *d_init_fir = nullptr;    // the caller's memory
};

// conceal mode: the composed record of a concealed stream, what dvda_mlp_hip_stream_info reports for it
struct ConcealInfo {
    uint32_t valid, status;
    uint64_t rows, frames;
};

// conceal mode (mlp_conceal.h): nothing of it is allocated before a batch with damage needs it
struct ConcealState {
    bool on = false;
    dvda_mlp_hip_ctx *child = nullptr;      // the second index: the kept ranges, each a stream of its own, fresh state
    DevBuf<ConcealPlan> d_plan;
    DevBuf<uint8_t> d_bytes;                // the ranges gathered 16-byte aligned (+ 64 readable bytes)
    DevBuf<uint64_t> d_tab;                 // gather table [3 * pieces], then the child's ranges and outputs [4 * pieces]
    DevBuf<int32_t> d_scr[CONCEAL_ROUNDS];  // per round: the ranges' PCM, each laid out as the stream it belongs to
    DevBuf<ConcealOp> d_ops;
    DevBuf<int32_t> d_fir;                  // zero FIR history of the ranges' fresh decoders [pieces][2][48]
    DevBuf<int32_t> d_edge_fir;             // FIR history behind each range of a round [pieces][2][48] (k_conceal_edge_fir); only grows
    bool ran = false;                       // the last decode call ran in conceal mode (dvda_mlp_hip_conceal_edges)
    std::vector<StreamRec> h_streams;       // ... and the stream records it read
    std::vector<dvda_mlp_conceal_edges> edges;              // per stream of the last decode: the damaged ones (valid: reserved = 1)
    std::vector<std::vector<dvda_mlp_conceal_span>> spans;  // per stream of the last decode
    std::vector<ConcealInfo> info;                           // per stream of the last decode: the concealed ones

    ~ConcealState() { dvda_mlp_hip_destroy(child); }
};

// presentation (mlp_present.h): nothing of it exists before dvda_mlp_hip_set_presentation asks for substream 0
struct PresentState {
    uint32_t mode = DVDA_PRESENT_FULL;      // DVDA_PRESENT_*
    dvda_mlp_hip_ctx *child = nullptr;      // the second index and every decode pass: the presentation streams
    DevBuf<uint8_t> d_bytes;                // the presentation streams, each 16-byte aligned (+ 64 readable bytes); only grows
    uint64_t bound = 0;                     // bytes of it the second index scans
    DevBuf<uint32_t> d_info;                // [max_streams]: k / why there is no presentation (PP_*)
    DevBuf<uint32_t> d_size;                // [max_segments + 1]: stripped bytes per source segment
    DevBuf<uint32_t> d_sbase;               // [max_segments + 1]: their exclusive prefix sum
    DevBuf<uint32_t> d_len;                 // [max_streams + 1]: the streams' lengths, padded to 16
    DevBuf<uint32_t> d_base;                // [max_streams + 1]: the streams' offsets; last = bytes in use
    DevBuf<uint64_t> d_off64, d_len64;      // [max_streams]: the ranges as the second index reads them
    Event ev[2];                            // around the strip kernels of the last index call
    bool ev_set = false;
    // host copies for the getters, fetched on first use after an index call
    bool map_valid = false;
    uint32_t h_nseg = 0;
    std::vector<SegRec> h_seg;
    std::vector<uint32_t> h_sbase, h_base, h_info;
    std::vector<StreamRec> h_streams;

    ~PresentState() { dvda_mlp_hip_destroy(child); }
};

struct dvda_mlp_hip_ctx {
    int device;
    uint32_t coop_min_seg;     // DecodeArgs::coop_min_seg: 1.75 waves per SIMD of this device (measured: slower at 1.5, 4.5 % faster at 2) (DVDA_COOP_MIN_SEG overrides: diagnostic)
    uint32_t max_streams, max_segments;
    // index workspace
    DevBuf<uint8_t> d_masks;            // [chunks]; grows with the input, and d_parts with it
    DevBuf<uint16_t> d_parts;           // [chunks + 72]: per 16-byte chunk, CRC-8 from state 0 | XOR of its bytes << 8 (mlp_check.h)
    DevBuf<uint32_t> d_tile_count;      // [tiles + 1]; grows with the input, and d_tile_base with it
    DevBuf<uint32_t> d_tile_base;       // [tiles + 1]; last = number of candidates
    DevBuf<uint64_t> d_cand_off;        // [max_segments]
    DevBuf<SegRec> d_seg;               // [max_segments]
    DevBuf<uint32_t> d_seg_frames;      // [max_segments + 1]
    DevBuf<uint32_t> d_seg_fbase;       // [max_segments + 1]
    DevBuf<uint32_t> d_seg_status;      // [max_segments]
    DevBuf<uint32_t> d_seg_rows;        // [max_segments]
    DevBuf<StreamRec> d_streams;        // [max_streams]
    uint32_t *d_n_cand;                 // single counter (points at d_tile_base[tiles])
    DevBuf<uint32_t> d_scan_tmp;        // block sums of the multi-block scans
    DevBuf<int32_t> d_iir;
    DevBuf<uint32_t> d_mat;
    DevBuf<unsigned long long> d_dbg;
    DevBuf<int32_t> d_fir;
    DevBuf<uint32_t> d_seg_meta;        // [iir_lanes]: channel range per (segment, substream) at the segment's end
    DevBuf<uint32_t> d_yield;           // [max_segments]: yield requests of the fast pass (mlp_decode.h, ST_YIELD)
    DevBuf<uint32_t> d_seg_check;       // [2 * max_segments]: parity / CRC-8 verdict per (segment, substream) (mlp_check.h)
    DevBuf<uint32_t> d_cls;             // [2]: streams with one / two substreams in the batch; [2] = the batch mixes shapes
    DevBuf<uint32_t> d_shape_key;       // [max_streams]
    DevBuf<uint64_t> d_soff, d_slen;    // [max_streams]: the caller's stream ranges as the index uses them (k_check_ranges)
    DevBuf<uint32_t> d_rank;            // [max_streams]
    DevBuf<uint32_t> d_sorted_cnt;      // [max_streams + 1]
    DevBuf<uint32_t> d_sorted_base;     // [max_streams + 1]
    DevBuf<uint32_t> d_lane_seg;        // [max_segments]
    DevBuf<DecodeSummary> d_summary;
    DecodeSummary *h_summary;  // pinned
    Stream st_aux;                      // the index's side branch: lane packing beside k_au_check (round 5)
    Event ev_fork, ev_join;
    DevBuf<uint32_t> d_seq_list;        // [max_streams]: streams for the sequential pass
    DevBuf<uint4> d_plan;               // [max_segments + 1]
    DevBuf<uint4> d_scan4_tmp;          // [max_segments / 1024 + 2]
    DevBuf<uint32_t> d_def_list;        // [max_segments]
    DevBuf<uint32_t> d_head_list;       // [max_segments]
    DevBuf<uint32_t> d_chain_order;     // [max_segments]: the chains, longest first
    DevBuf<uint32_t> d_chain_hist;      // [2 * CHAIN_BUCKETS]
    // grown on first use (a batch that needs them):
    DevBuf<int32_t> d_fb;               // sequential pass: one frame buffer (FB_WORDS) per lane pair of a round
    uint32_t rsv_segs;                  // dvda_mlp_hip_reserve: deferred segments a non-blocking decode launches its chain passes for
    DevBuf<int32_t> d_res;              // chain passes: planes
    DevBuf<uint32_t> d_brec;
    DevBuf<uint32_t> d_frec;
    uint32_t iir_lanes;
    // the six dvda_mlp_hip_pcm_* calls (pcm_report_run.h, report_of_decode): grown on first use, and the same three for
    // every report.  What one report left in them is the next one's to overwrite: a report reads
    // no word of the workspace or the result block that the same call has not stored (the tests named
    // test_poisoned_workspace and test_deterministic_on_a_poisoned_workspace pin that).
    DevBuf<dvda_pcm_crc_desc> d_rep_desc;   // [streams], and behind them the descriptors a report stages of its own
    DevBuf<uint64_t> d_rep_out;         // the results and what a report lays behind them (its stage() / bind())
    DevBuf<uint32_t> d_rep_work;
    DecodeSettings set;
    // call state
    const uint8_t *d_bytes;
    uint64_t total_bytes;
    const uint64_t *d_stream_off;
    const uint64_t *d_stream_len;
    uint32_t n_streams;
    uint64_t tiles;
    bool indexed;
    bool small_input;          // the last index call's input was at most SMALL_INPUT_BYTES
    bool decoded;              // a decode call has run on the current index (the next one resets the segments first)
    // the index's launch sequence as a hipGraph, replayed while a caller indexes the same buffers again and
    // again (a pipeline that reuses its staging buffers, the bench): one graph launch instead of ~18 launches
    GraphExec idx_graph;
    const void *idx_key[4];    // d_bytes, d_stream_off, d_stream_len, stream of the captured / last call
    uint64_t idx_key_bytes;
    uint32_t idx_key_streams;
    int idx_graph_state;       // 0: off / not yet, 1: the key was seen once (capture on the next match), 2: captured, -1: disabled
    // timing of the fast-pass kernel: a fixed ring of (start, stop) pairs made at create time
    Event ev[2 * EV_RING];
    Event ev_end[EV_RING];     // behind the last kernel of the decode call (dvda_mlp_hip_decode_time)
    uint64_t ev_count;         // decode calls recorded since the last dvda_mlp_hip_kernel_time
    ConcealState cc;
    PresentState pp;

    uint32_t fb_slots() const { return (uint32_t)(d_fb.cap / FB_WORDS); }
    ~dvda_mlp_hip_ctx() { (void)hipHostFree(h_summary); }
};

// what the workspaces hold right now (mlp_bounds.h)
static WsCaps ws_caps(const dvda_mlp_hip_ctx *c)
{
    WsCaps w;
    w.res = c->d_res.cap;
    w.brec = c->d_brec.cap;
    w.frec = c->d_frec.cap;
    w.fb = c->d_fb.cap;
    w.max_seg = c->max_segments;
    w.max_streams = c->max_streams;
    w.lanes = c->iir_lanes;
    w.pad = 0;
    return w;
}

// presentation: the decode passes and their timers are the inner context's (null: there is none, or the mode is off)
static inline dvda_mlp_hip_ctx *pp_inner(const dvda_mlp_hip_ctx *c)
{
    return c && c->pp.mode == DVDA_PRESENT_SUBSTREAM0 ? c->pp.child : nullptr;
}

// what a stream's major sync says of it, as the packed word the index keeps (StreamRec::sync)
static inline void fill_sync_fields(dvda_mlp_stream_info &o, uint32_t sync)
{
    o.assignment = (sync >> 16) & 0x1F;
    o.substreams = (sync >> 24) & 0xF;
    o.group0_bps = sync & 0xF;
    o.group1_bps = (sync >> 4) & 0xF;
    o.group0_rate = (sync >> 8) & 0xF;
    o.group1_rate = (sync >> 12) & 0xF;
}

// exclusive scan of n (host count, or *n_ptr clamped to n_cap) uint32 values on `st`; out[n] = total.
// tmp: block sums of the multi-block form, (n + 1023) / 1024 + 2 words
static void enqueue_exscan(hipStream_t st, const uint32_t *in, uint32_t *out, uint32_t *tmp, uint32_t n_host,
                           const uint32_t *n_ptr, uint32_t n_cap)
{
    const uint32_t n_max = n_ptr ? n_cap : n_host;
    if (n_max <= 4096) {
        hipLaunchKernelGGL(k_exscan_u32, dim3(1), dim3(1024), 0, st, in, out, n_host, n_ptr, n_cap);
        return;
    }
    const uint32_t blocks = (n_max + 1023) / 1024;
    hipLaunchKernelGGL(k_scan_blocks, dim3(blocks), dim3(1024), 0, st, in, out, tmp, n_host, n_ptr, n_cap);
    // bases of the blocks, in place; the total lands at tmp[blocks]
    hipLaunchKernelGGL(k_exscan_u32, dim3(1), dim3(1024), 0, st, tmp, tmp, blocks, (const uint32_t *)nullptr, blocks);
    hipLaunchKernelGGL(k_scan_add, dim3(blocks), dim3(1024), 0, st, out, tmp, blocks, n_host, n_ptr, n_cap);
}
