/* dvda_mlp_hip.h -- C ABI of the MI355X-native MLP decode path.
 *
 * This is the drop-in boundary for the ONE hot path of tuffy/libdvd-audio:
 * MLP (Meridian Lossless Packing) access-unit decode.  Everything a binding
 * needs is plain C: pointers, sizes and opaque handles -- no C++/HIP/torch
 * types.  Pointers named d_* are DEVICE pointers (HBM); `stream` is a
 * hipStream_t passed as void* (NULL = default stream).
 *
 * Two tiers:
 *
 *  (A) Batch tier -- the fast path.  Many independent MLP byte streams (titles,
 *      tracks, or single access units) resident in HBM are framed, parsed,
 *      filtered, rematrixed and written as planar int32 PCM in RIFF-WAVE
 *      channel order by hand-written gfx950 kernels.  It replaces, for a whole
 *      batch at once, what the reference does one PES payload at a time in
 *        dvda_mlpdecoder_decode_packet()   reference src/mlp.h:39-42, src/mlp.c:344-354
 *        mlpdecoder_decode/read_mlp_frame  reference src/mlp.c:360-405   (framing)
 *        decode_mlp_frame                  reference src/mlp.c:407-612   (sync, substreams,
 *                                                                          rematrix, shift, order)
 *        decode_substream .. filter_channel reference src/mlp.c:714-1306 (parse + FIR/IIR)
 *        rematrix_channels                 reference src/mlp.c:1308-1358
 *        checkdata_callback                reference src/mlp.c:1360-1399 (parity / CRC-8)
 *
 *  (B) Streaming tier -- the mlp.h mirror (declared further below):
 *      dvda_hip_open_mlpdecoder / dvda_hip_mlpdecoder_decode_packet /
 *      dvda_hip_close_mlpdecoder keep the exact call shape and return-value
 *      meaning of reference src/mlp.h:29-42 with the reference's BitstreamReader
 *      and aa_int containers replaced by (pointer, length) pairs; INTEGRATION.md
 *      shows the 40-line src/mlp.c replacement that binds them.  A host that
 *      serves many streams at once opens a group of such decoders
 *      (dvda_hip_open_mlpdecoder_group): one call feeds every member its
 *      packet, and all of them are decoded by one launch pair.
 *
 * All functions return 0 on success or a negative DVDA_HIP_E* code; they never
 * fall back to a CPU implementation.
 */
#ifndef DVDA_MLP_HIP_H
#define DVDA_MLP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVDA_HIP_OK          0
#define DVDA_HIP_ENODEV     -1   /* no usable HIP device / HIP runtime error */
#define DVDA_HIP_ENOMEM     -2
#define DVDA_HIP_EINVAL     -3
#define DVDA_HIP_ECAPACITY  -4   /* more streams / segments / bytes than the context was created for */
#define DVDA_HIP_ESTATE     -5   /* call order violated (decode before index, ...) */

/* per-stream / per-segment status bits (0 = decoded exactly as the reference
 * decodes a well-formed stream).  The low 10 bits mirror oracle/mlp_oracle.h. */
#define DVDA_ST_NO_SYNC      (1u << 0)   /* stream does not begin with a major sync             */
#define DVDA_ST_SYNC_CHANGE  (1u << 1)   /* a later major sync carries other stream parameters: that access
                                            unit was dropped and decoding went on, as the reference does
                                            (src/mlp.c:449-460) -- informational; together with
                                            DVDA_ST_IRREGULAR: could not be resolved, not decoded        */
#define DVDA_ST_PARITY       (1u << 2)
#define DVDA_ST_CRC          (1u << 3)
#define DVDA_ST_EOF          (1u << 4)   /* parse ran past a substream / frame end               */
#define DVDA_ST_RESTART      (1u << 5)   /* bad restart header                                   */
#define DVDA_ST_PARAMS       (1u << 6)   /* bad decoding parameters                              */
#define DVDA_ST_HUFFMAN      (1u << 7)   /* invalid residual code                                */
#define DVDA_ST_FILTER       (1u << 8)   /* FIR+IIR order > 8 or shift mismatch                  */
#define DVDA_ST_ENVELOPE     (1u << 9)   /* stream outside the reference's defined behaviour     */
/* conditions the batch tier reports instead of guessing: */
#define DVDA_ST_IRREGULAR    (1u << 16)  /* frame chain does not land on the next major sync     */
#define DVDA_ST_TIMING       (1u << 17)  /* an access unit's PCM-frame count differs from the
                                            stream's standard 40/80/160: stream decoded in order
                                            by the sequential pass                               */
#define DVDA_ST_MIDFRAME     (1u << 18)  /* matrix-class parameters changed after a frame's
                                            first block: segment decoded by the chain passes
                                            (rematrix per access unit, src/mlp.c:504-525)        */
#define DVDA_ST_CHAINED      (1u << 19)  /* segment's first block uses the FIR history of the
                                            previous segment (the reference never clears it):
                                            decoded by the chain passes                          */
#define DVDA_ST_OVERFLOW     (1u << 20)  /* output capacity (out_stride) too small               */
#define DVDA_ST_TRUNCATED    (1u << 21)  /* stream ends inside a frame (tail not consumed)       */
#define DVDA_ST_CAPACITY     (1u << 22)  /* more major syncs than max_segments: the stream (and those behind
                                            it) were indexed only in part -- create a larger context     */
#define DVDA_ST_GENERAL      (1u << 23)  /* segment was decoded by a pass behind the fast pass (informational) */
#define DVDA_ST_FALSE_SYNC   (1u << 24)  /* segment-level only: a sync pattern inside another segment's
                                            frame chain (payload / padding bytes), resolved and skipped */
#define DVDA_ST_SEQ          (1u << 25)  /* a restart header inside an access unit, or very dense parameter
                                            changes in a segment of the chain passes: stream decoded in
                                            order by the sequential pass                                  */
#define DVDA_ST_COLD         (1u << 26)  /* IIR taps, or more than two matrices: the fused row loop keeps
                                            neither in registers -- segment decoded by the chain passes   */
#define DVDA_ST_YIELD        (1u << 27)  /* the segment in front of a chained one (or one of the few segments
                                            without a chain among many with one), decoded by the chain passes
                                            with them instead of alone by the fast pass (informational)  */
#define DVDA_ST_DEVICE       (1u << 29)  /* streaming tier only: a HIP runtime call failed inside a step -- not a
                                            property of the stream; the decoder stops (it does not fall back to the
                                            batch tier on the same device without a word)                     */
#define DVDA_ST_CONCEALED    (1u << 30)  /* conceal mode only (dvda_mlp_hip_set_conceal): the stream was damaged and
                                            comes out as kept PCM, silence and PCM of a fresh decoder; the damage
                                            bits moved into its spans (dvda_mlp_hip_conceal_spans).  NOT in
                                            DVDA_ST_BENIGN: a caller has to ask for silence to accept it      */
/* DVDA_ST_CHAINED, _MIDFRAME, _COLD, _YIELD, _TIMING and _SEQ are raised by the fast pass and then decoded exactly by
 * the passes behind it (chain passes: parse in parallel, the filter recursion alone per channel, rematrix
 * in parallel; or the sequential pass); they stay set as information.  Bits that do not invalidate the PCM: */
#define DVDA_ST_BENIGN (DVDA_ST_TRUNCATED | DVDA_ST_CHAINED | DVDA_ST_MIDFRAME | DVDA_ST_TIMING | DVDA_ST_GENERAL | \
                        DVDA_ST_SEQ | DVDA_ST_SYNC_CHANGE | DVDA_ST_COLD | DVDA_ST_YIELD)

typedef struct dvda_mlp_hip_ctx dvda_mlp_hip_ctx;

typedef struct dvda_mlp_stream_info {
    uint64_t mlp_frames;      /* complete access units that yield PCM: those of the live segments without
                                 the units dropped for a major sync with other parameters
                                 (DVDA_ST_SYNC_CHANGE); bytes_consumed covers the dropped ones too          */
    uint64_t pcm_frames;      /* PCM frames decoded per channel                               */
    uint64_t bytes_consumed;  /* bytes covered by complete access units                       */
    uint32_t status;          /* DVDA_ST_* bits                                               */
    uint32_t channels;        /* channel count of the stream's channel assignment            */
    uint32_t substreams;      /* 1 or 2 (from the first major sync)                           */
    uint32_t assignment;      /* 5-bit channel assignment                                     */
    uint32_t group0_bps, group1_bps, group0_rate, group1_rate;  /* major sync codes          */
    uint32_t segments;        /* major-sync candidates the stream has in the segment list, from its first one
                                 to the last in front of the next stream's: the restart-delimited segments
                                 (units of parallel decode) AND the retired ones (DVDA_ST_FALSE_SYNC) among
                                 them -- the length of the stream's run of segment indices                  */
    uint32_t reserved;
} dvda_mlp_stream_info;

/* ------------------------------------------------------------------ tier A */

/* Creates a decode context on HIP device `device` able to hold an index for up
 * to max_streams streams / max_segments restart segments.  The workspace of the index and of the
 * fast pass is allocated here.  A batch that needs the passes behind the fast pass (chained FIR
 * history, mid-frame parameter changes, non-standard timing) grows their workspace on first use
 * inside dvda_mlp_hip_decode. */
int dvda_mlp_hip_create(dvda_mlp_hip_ctx **ctx, int device, uint32_t max_streams,
                        uint32_t max_segments);
void dvda_mlp_hip_destroy(dvda_mlp_hip_ctx *ctx);

/* Frame index (reference src/mlp.c:384-405 + the major-sync test of :614-654):
 * finds every major-sync access unit, walks the 12-bit size chain between
 * them, and derives each segment's first output row.  d_bytes must be readable
 * for total_bytes + 64 bytes; stream i occupies
 * [d_stream_off[i], d_stream_off[i] + d_stream_len[i]) and starts 16-byte aligned; the streams' ranges are
 * ascending and do not overlap (a major sync belongs to the one stream whose range holds it).  The ranges are
 * checked on the device: a stream that starts before the end of a stream in front of it (of two streams given
 * the same bytes, the second), is misaligned or leaves the buffer is not decoded and carries
 * DVDA_ST_IRREGULAR (| DVDA_ST_ENVELOPE) -- never a walk outside the buffer. */
/* (A caller that indexes the same buffers again and again -- a pipeline that reuses its staging buffers -- gets
 * the index's launch sequence replayed as one hipGraph from the third such call on; `stream` must then be a
 * real stream, not NULL.  DVDA_INDEX_GRAPH=0 in the environment switches that off.) */
int dvda_mlp_hip_index(dvda_mlp_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t total_bytes,
                       const uint64_t *d_stream_off, const uint64_t *d_stream_len,
                       uint32_t n_streams, void *stream);

/* Decodes every indexed segment.  Stream i's PCM is written planar at
 * d_pcm[d_out_off[i] + channel * d_out_stride[i] + pcm_frame], channel in
 * RIFF-WAVE order (reference src/mlp.c:416-438, 527-533).
 * The call waits once on `stream` for the fast pass: a 32-byte summary tells the host whether the
 * chain passes / the sequential pass have anything to do (they are not launched otherwise); what it
 * enqueues after that is asynchronous again.
 * An index may be decoded more than once (a caller that comes back with a larger buffer after
 * DVDA_ST_OVERFLOW, or wants the titles in a second buffer): every call starts from what the index left,
 * nothing of the call before it is carried over. */
int dvda_mlp_hip_decode(dvda_mlp_hip_ctx *ctx, int32_t *d_pcm, const uint64_t *d_out_off,
                        const uint64_t *d_out_stride, void *stream);

/* The same without the host ever waiting and without any allocation: every pass is enqueued on `stream` and the call
 * returns -- so a caller can have the index of the next batch running (another context, another stream) while this
 * batch decodes, or capture the call.  What the fast pass defers is decoded on the workspaces dvda_mlp_hip_reserve
 * left: the chain passes are launched for as many deferred segments / PCM frames as were reserved and find their
 * work on the device, the sequential pass for as many streams as were reserved; a batch that needs more than was
 * reserved is NOT decoded short silently -- the streams left over carry DVDA_ST_CAPACITY (dvda_mlp_hip_stream_info),
 * and the blocking call or a larger reservation decodes them.  With nothing reserved (a batch of regular titles with
 * raw lead-in blocks at their restart points) only the fast pass and two small bookkeeping kernels are launched.
 * Host-blocking entry points are dvda_mlp_hip_decode (once per call, twice when chains exist; it also grows the
 * workspaces on first use) and the *_info / *_count calls. */
int dvda_mlp_hip_decode_async(dvda_mlp_hip_ctx *ctx, int32_t *d_pcm, const uint64_t *d_out_off,
                              const uint64_t *d_out_stride, void *stream);
/* (On a context in conceal mode dvda_mlp_hip_decode_async returns DVDA_HIP_EINVAL: concealing reads the damage back.) */

/* Conceal mode (default off; off = every output, status bit, launch and allocation as without it).  With it on,
 * dvda_mlp_hip_decode hands out a damaged stream as
 *     kept PCM ++ silence ++ PCM decoded by a fresh decoder ++ ...
 * instead of a non-benign status:
 *   damage   an access unit whose parity / CRC-8 fails or that cannot be framed; when no unit check locates it, the
 *            whole segment whose decode reported a non-benign status (always so for streams without check data)
 *   kept     every access unit in front of the first damaged one, exactly as without conceal mode (a range that starts at
 *            the stream's first byte is decoded with the FIR history dvda_mlp_hip_set_initial_fir gave the stream)
 *   resume   the first major sync behind the damage at which every substream opens with a restart header; from there
 *            a fresh decoder (zero FIR / IIR history, no parameters carried) -- the PCM the reference returns for the
 *            bytes from that sync on.  Damage behind it: the same again (at most 4 decode rounds; what is still
 *            damaged after the last is concealed whole)
 *   reach    the first round is the caller's decode; each of the three behind it decodes the ranges planned so far.  A
 *            plan holds 16 ranges, the last of them open to the stream's end and planned again after its own decode.  So
 *            with damage that the units' checks locate a stream keeps 45 ranges, and a 46th when nothing behind it is
 *            damaged; what lies behind is one span with DVDA_CONCEAL_ROUNDS.  Damage behind a resume point that only the
 *            range's own decode finds (no check data) costs that range one round more
 *   silence  g = (t_r - t_k - n_k) mod 65536 PCM frames between the last kept unit (16-bit input timing t_k, n_k
 *            frames) and the resume unit (t_r), plus 65536 w, w >= 0 the integer that brings the span's bytes per
 *            frame closest to the stream's mean over its kept ranges; 0 frames in front of the first usable major
 *            sync and behind the last kept unit.  Zeros in every layout.
 *            (t_k + n_k is taken as the input timing of the kept range's first unit + the PCM frames the range decodes
 *            to: the last unit's own frame count, standard or not, without a second parse; input timing that does not
 *            advance by the units' PCM frames inside a kept range gives a gap off by the difference)
 * A concealed stream's status is DVDA_ST_CONCEALED | the benign bits of its kept ranges (| DVDA_ST_OVERFLOW when the
 * composed stream does not fit: pcm_frames = the capacity needed, and the stream's region holds no concealed output --
 * what the ordinary decode wrote there is left as it is); mlp_frames counts the kept access units.  These are what
 * dvda_mlp_hip_stream_info reports; the index's own records stay as the decode left them, so a second decode of the same
 * index (after DVDA_ST_OVERFLOW) starts from the index's findings, conceal mode on or off.  A stream without damage
 * decodes exactly as without conceal mode.  The call blocks a little longer for a batch with damage (a second index and
 * decode of the ranges); a clean batch costs one read of the stream records. */
int dvda_mlp_hip_set_conceal(dvda_mlp_hip_ctx *ctx, int on);

/* One concealed span of a stream: PCM frames [first_frame, first_frame + frames) of the output are silence, standing
 * for bytes [byte_off, byte_end) of the stream (offsets from the stream's first byte); cause = the DVDA_ST_* bits of the
 * damage.  flags: */
#define DVDA_CONCEAL_LEADING  1u    /* in front of the first usable major sync (frames = 0)           */
#define DVDA_CONCEAL_TRAILING 2u    /* behind the last kept access unit (frames = 0)                  */
#define DVDA_CONCEAL_ROUNDS   4u    /* holds a range still damaged after the last decode round        */
typedef struct dvda_mlp_conceal_span {
    uint64_t first_frame, frames;
    uint64_t byte_off, byte_end;
    uint32_t cause, flags;
} dvda_mlp_conceal_span;
/* The spans of `stream` from the last dvda_mlp_hip_decode in conceal mode (blocks on `stream_`): up to cap of them into
 * spans, *n = how many there are (0 for a clean stream). */
int dvda_mlp_hip_conceal_spans(dvda_mlp_hip_ctx *ctx, uint32_t stream, dvda_mlp_conceal_span *spans, uint32_t cap,
                               uint32_t *n, void *stream_);
/* The edges of `stream` after the last dvda_mlp_hip_decode in conceal mode: what a caller that feeds a long stream piece by
 * piece needs to join two pieces (blocks on `stream_`).  Valid for clean streams too: kept_begin 0, kept_end =
 * bytes_consumed, fir = that of the last live segment.  DVDA_HIP_ESTATE when the last decode was not in conceal mode.  A
 * clean stream costs a few small copies and no launch; the history behind each range of a damaged stream was gathered in
 * the round that decoded the range (csrc/mlp_conceal.h, k_conceal_edge_fir: one small launch, one copy of 96 words per
 * range to the host and one more blocking wait per round -- for batches with damage only). */
typedef struct dvda_mlp_conceal_edges {
    uint64_t kept_begin, kept_end; /* offsets from the stream's first byte: the first kept unit, and behind the last kept unit
                                      (kept_begin == kept_end: nothing kept) */
    uint32_t t_first, t_end;       /* 16-bit input timing of the first kept unit; behind the last one (t_first of the last
                                      range + its PCM frames, mod 65536) */
    uint64_t kept_bytes, kept_frames; /* sums over the kept ranges (for the caller's running mean) */
    uint32_t ends_kept;            /* 1: the last kept range runs to the stream's end (no TRAILING span) */
    uint32_t reserved;
    int32_t  fir[2 * 48];          /* FIR history behind the last kept unit, layout of dvda_mlp_hip_segment_fir (entries of
                                      channel slots a substream does not have are undefined there and here) */
} dvda_mlp_conceal_edges;
int dvda_mlp_hip_conceal_edges(dvda_mlp_hip_ctx *ctx, uint32_t stream, dvda_mlp_conceal_edges *out, void *stream_);

/* Presentation (default DVDA_PRESENT_FULL; with it every output, status bit, launch and allocation is as without this
 * call, also after DVDA_PRESENT_SUBSTREAM0 was set and taken back).
 *
 * A two-substream MLP stream carries two presentations: substream 0 alone is the 2-channel one (k channels in general:
 * its own restart headers, filters, matrices and output shifts -- what a 2-channel decoder plays from a multichannel
 * disc), both substreams together the full one.  The reference, and DVDA_PRESENT_FULL, parse substream 0's matrices
 * and never apply them for such a stream (src/mlp.c:539-609): channels 0 and 1 of the full decode are front left and
 * right, not the stereo mix.  DVDA_PRESENT_SUBSTREAM0 decodes the *presentation stream* of every stream instead:
 *
 *   one substream    the stream itself, byte for byte
 *   two substreams   per complete access unit of the frame chain, in order:
 *     frame header   the 4 check bits and the 16-bit input timing kept; the 12-bit length = the new unit's 16-bit words
 *     major sync     (when the unit has one) its 28 bytes with the substream count set to 1 and the 5-bit channel
 *                    assignment set to the identity assignment of k channels -- k = 1: 0x00, 2: 0x01, 3: 0x02, 4: 0x03,
 *                    5: 0x06, which map MLP channel c to RIFF channel c (src/mlp.c:416-438).  k = substream 0's
 *                    max_matrix_channel + 1 from the restart header of the stream's FIRST unit (bits 40-43 of substream
 *                    0's bytes when both leading flags are set, src/mlp.c:748-753, 822-826); a first unit whose
 *                    substream 0 opens with no restart header, or a k above 5: DVDA_ST_ENVELOPE, nothing decoded
 *     directory      substream 0's word (and its extra word) kept, substream 1's dropped
 *     body           bytes [0, 2 * substream_end_0) of the substream area, the rest dropped; a range that does not fit
 *                    in the unit is clamped to it (the decode's own checks then report the damage)
 *
 * which is an ordinary one-substream stream (src/mlp.c:504-538; substream 0's parity and CRC-8 cover its own bytes
 * only and stay valid).  PCM, status, pcm_frames, mlp_frames and segments are those of that stream: damage confined to
 * substream 1's bytes does not touch the presentation, and a later restart header whose max_matrix_channel disagrees
 * with k is judged as in any one-substream stream.
 *
 * With it set, dvda_mlp_hip_index indexes the source, strips it on the device into a workspace that only grows
 * (csrc/mlp_present.h; no host wait) and indexes the presentation streams with a second, inner context.
 * dvda_mlp_hip_decode / _decode_async / _reserve / _set_pcm_layout / _set_initial_fir (substream 0's history is
 * [stream][0][..]) / _set_lanes_per_segment / _set_chain_form / _kernel_time / _decode_time / _segment_count /
 * _segment_fir act on that context, so every pass and all four layouts work as for any one-substream stream.
 *   dvda_mlp_hip_stream_info   channels = k (right after the index), pcm_frames, mlp_frames, segments and status are
 *                              the presentation's; substreams, assignment and the group codes stay the source's;
 *                              bytes_consumed counts source bytes.  A source stream the index could not frame
 *                              (DVDA_ST_NO_SYNC, _IRREGULAR, _CAPACITY) keeps that status and decodes nothing.
 *   dvda_mlp_hip_segment_info  segments are the presentation streams'; offset and end are positions in the caller's
 *                              SOURCE buffer (the start of the source segment whose stripped bytes begin there).
 * Scope: conceal mode and DVDA_PRESENT_SUBSTREAM0 on one context give DVDA_HIP_EINVAL, whichever is set second; the
 * streaming tier and dvda_mlp_hip_decode_multi decode the full presentation only; a batch of 4 GiB or more is
 * DVDA_HIP_ECAPACITY under DVDA_PRESENT_SUBSTREAM0 (offsets in the workspace are 32-bit).  A change of the setting
 * asks for a new dvda_mlp_hip_index. */
#define DVDA_PRESENT_FULL        0u
#define DVDA_PRESENT_SUBSTREAM0  1u
int dvda_mlp_hip_set_presentation(dvda_mlp_hip_ctx *ctx, uint32_t presentation);
/* Device time (ms) of the strip kernels of the last dvda_mlp_hip_index under DVDA_PRESENT_SUBSTREAM0, the source bytes
 * they walked and the bytes of the presentation streams they wrote (blocks until they have run). */
int dvda_mlp_hip_present_time(dvda_mlp_hip_ctx *ctx, double *ms, uint64_t *bytes_in, uint64_t *bytes_out);
/* Diagnostic: the presentation buffer of the last dvda_mlp_hip_index under DVDA_PRESENT_SUBSTREAM0, read back to the host
 * (blocks on `stream`; changes nothing in the context).  Every argument but ctx may be NULL / 0:
 *   offsets, lengths   [n] (n clamped to the streams of the index): where presentation stream i starts in the buffer
 *                      (a multiple of 16: the running sum of the lengths in front of it, each rounded up to 16) and its
 *                      length in bytes -- 0 for a stream that has no presentation
 *   readable           bytes of the buffer the call hands out: what the second index is told to scan (the source's
 *                      total_bytes rounded up to 16, plus 16 per stream) and the 64 bytes behind it that it may read.
 *                      All of them behind the end of a stream -- the padding up to the next stream's start, and
 *                      everything behind the last stream -- are zero
 *   bytes              [count]: bytes [first, first + count) of the buffer; first + count > readable: DVDA_HIP_EINVAL
 * DVDA_HIP_ESTATE unless the context is indexed under DVDA_PRESENT_SUBSTREAM0. */
int dvda_mlp_hip_present_read(dvda_mlp_hip_ctx *ctx, uint64_t *offsets, uint64_t *lengths, uint32_t n, uint64_t *readable,
                              uint8_t *bytes, uint64_t first, uint64_t count, void *stream);

/* Sizes the workspaces of the passes behind the fast pass ahead of time (they only ever grow): chain passes for
 * `chain_segments` deferred segments holding `chain_pcm_frames` PCM frames in all (for titles whose restart points
 * carry FIR taps -- what encoders write -- that is every segment and every frame of the batch), the sequential pass
 * for `seq_streams` streams at a time.  After it neither decode call allocates for a batch within these sizes. */
int dvda_mlp_hip_reserve(dvda_mlp_hip_ctx *ctx, uint64_t chain_pcm_frames, uint32_t chain_segments,
                         uint32_t seq_streams);

/* PCM layout of dvda_mlp_hip_decode (default DVDA_PCM_PLANAR, above).  DVDA_PCM_INTERLEAVED writes
 * frame-major instead: d_pcm[d_out_off[i] + pcm_frame * channels + channel] -- the order the
 * reference's dvda_read() hands out (src/dvd-audio.c:781-792); d_out_stride[i] stays the capacity
 * in PCM frames, so stream i occupies channels * d_out_stride[i] values either way.  Same sample
 * values; each lane's stores become one contiguous run, which the memory side takes much better
 * (6-channel titles: 5-8 % faster, 40 % less write traffic; 2-channel: the same speed; other channel
 * counts: a few per cent slower than planar -- DESIGN.md section 4). */
#define DVDA_PCM_PLANAR      0u
#define DVDA_PCM_INTERLEAVED 1u
/* The output stage fused into the decode: d_pcm receives the interleaved little-endian
 * WAV payload dvda2wav writes -- frame-major like DVDA_PCM_INTERLEAVED, every value as write_signed(24) /
 * write_signed(16) (reference utils/dvda2wav.c:326-334, src/bitstream.c:2846-2857: low bits - 1 bits plus a
 * sign bit taken from v < 0).  Stream i's payload starts at byte 4 * d_out_off[i] of d_pcm (d_out_off stays in
 * int32 units, so every stream starts dword-aligned) and holds pcm_frames * channels * (3 | 2) bytes;
 * d_out_stride[i] stays the capacity in PCM frames.  Same bytes as dvda_mlp_hip_pack_wav() of the int32 PCM. */
#define DVDA_PCM_WAV24       2u
#define DVDA_PCM_WAV16       3u
int dvda_mlp_hip_set_pcm_layout(dvda_mlp_hip_ctx *ctx, uint32_t layout);

/* Blocks until the work enqueued on `stream` is done and copies the per-stream
 * results to host memory. */
int dvda_mlp_hip_stream_info(dvda_mlp_hip_ctx *ctx, dvda_mlp_stream_info *infos, uint32_t n,
                             void *stream);

/* Number of segments found by the last index call (blocks on `stream`). */
int dvda_mlp_hip_segment_count(dvda_mlp_hip_ctx *ctx, uint32_t *n_segments, void *stream);

/* How the last dvda_mlp_hip_index call's launches went out (read-only, no device work): *state is 0 before the
 * first index (or for one on the NULL stream before any other), 1 when the call's buffers, counts and stream were
 * noted and its kernels launched directly, 2 when the launch sequence was captured or replayed as a hipGraph,
 * -1 when the graph is switched off (DVDA_INDEX_GRAPH=0, or a capture / replay failed on this context). */
int dvda_mlp_hip_index_graph_state(dvda_mlp_hip_ctx *ctx, int *state);

/* Average duration in milliseconds of the fast-pass kernel launches recorded since
 * the last call (HIP events on the launch stream, a ring of the newest 256 decode calls made at
 * create time); *launches receives the count.  Blocks until those launches have finished. */
int dvda_mlp_hip_kernel_time(dvda_mlp_hip_ctx *ctx, double *avg_ms, uint32_t *launches);

/* The same ring read the other way: average device time of a whole decode call -- from the first kernel of the fast
 * pass to the last kernel the call enqueued (chain passes, sequential pass, bookkeeping; for the blocking call the
 * gaps while the host read the summary count too).  Does not reset the ring: call it before
 * dvda_mlp_hip_kernel_time. */
int dvda_mlp_hip_decode_time(dvda_mlp_hip_ctx *ctx, double *avg_ms, uint32_t *calls);

/* ------------------------------------------------------------------ several GPUs from one C host
 * titles are independent -- the reference decodes one track at a time through one decoder,
 * src/dvd-audio.c:597-657, and two decoders share nothing -- so a host with a list of streams gives every GPU its
 * own sub-list: greedy longest-processing-time on the compressed size (dvda_mlp_hip_shard, the same deterministic
 * partition as libdvd-audio_amd/shard.py), one host thread + decode context + HIP stream per device entry, no
 * exchange between devices, a small summary added up over RCCL -- or on the host, see `reduction` -- (csrc/mlp_multi.cpp).  The streams and the PCM are
 * HOST buffers here (each device gets its own copies); a device may be named more than once. */
typedef struct dvda_mlp_hip_multi dvda_mlp_hip_multi;
typedef struct dvda_mlp_multi_summary {
    uint64_t pcm_frames;                  /* sum over the streams                                         */
    uint64_t samples;                     /* sum of pcm_frames x channels                                 */
    uint64_t compressed_bytes;            /* sum of the stream lengths                                    */
    uint64_t compressed_bytes_max_device; /* the largest share one device entry got (load balance)        */
    uint32_t streams_with_errors;         /* streams whose status has a bit outside DVDA_ST_BENIGN        */
    uint32_t devices;                     /* device entries the list was dealt to                         */
    /* (round 5) what a caller needs to judge a run on N devices without a profiler: wall time of the slowest and the
     * fastest device entry (copy in + index + decode + copy out, its host thread's clock), and the load imbalance
     * of the deal = largest share of the compressed bytes / mean share (1.0 = even)                              */
    double device_ms_max;
    double device_ms_min;
    double imbalance;
    /* (round 6) who added the summary up: 1 = RCCL (one communicator per device, two all-reduces -- a device list that
     * names every device once, librccl present), 0 = the host (a device named twice, no librccl, DVDA_MULTI_RCCL=0) */
    uint32_t reduction;
    uint32_t reserved;
} dvda_mlp_multi_summary;

/* part_of[i] = which of `parts` parts stream i (sizes[i] bytes) goes to */
int dvda_mlp_hip_shard(const uint64_t *sizes, uint32_t n, uint32_t parts, uint32_t *part_of);
/* one decode context per entry of devices[]; every one sized for max_streams / max_segments */
int dvda_mlp_hip_create_multi(dvda_mlp_hip_multi **multi, const int *devices, uint32_t n_devices,
                              uint32_t max_streams, uint32_t max_segments);
void dvda_mlp_hip_destroy_multi(dvda_mlp_hip_multi *multi);
uint32_t dvda_mlp_hip_multi_devices(const dvda_mlp_hip_multi *multi);
/* wall time (ms) the last dvda_mlp_hip_decode_multi spent on device entry `entry`, and the compressed bytes it got */
int dvda_mlp_hip_multi_device_time(const dvda_mlp_hip_multi *multi, uint32_t entry, double *ms, uint64_t *bytes);
/* Decodes n_streams host streams (streams[i], lengths[i] bytes) and returns when all of them are done.  pcm[i]
 * receives stream i in `layout` (DVDA_PCM_*): planar = [channel][capacity_frames[i]] int32, interleaved =
 * [frame][channel] int32, WAV24 / WAV16 = the packed payload; capacity_frames[i] = PCM frames per channel pcm[i]
 * has room for (a stream that needs more is reported DVDA_ST_OVERFLOW, infos[i].pcm_frames = the size needed).
 * infos[i] as dvda_mlp_hip_stream_info would give it; summary may be NULL.  Blocks; no CPU fallback. */
int dvda_mlp_hip_decode_multi(dvda_mlp_hip_multi *multi, const uint8_t *const *streams, const uint64_t *lengths,
                              uint32_t n_streams, uint32_t layout, void *const *pcm, const uint64_t *capacity_frames,
                              dvda_mlp_stream_info *infos, dvda_mlp_multi_summary *summary);

/* Range-checked diagnostic build (-DDVDA_BOUNDS, tests/test_gpu_soak.py): every index a kernel forms into a
 * workspace of the library is compared with the workspace's size; out4 = {violations so far, and of the first
 * one: array tag, index, capacity}.  Returns 1 from a checked build, 0 from the shipped library (which does not
 * check and reports zeros), < 0 on error. */
int dvda_mlp_hip_bounds_violations(unsigned long long *out4);

/* Which fast-pass kernels run.  0 (default): chosen per batch from the substream counts the index
 * found -- streams with one substream take the one-lane-per-segment kernel, streams with two the kernel
 * whose lane reads both substreams of its segment (round 6; any split of the channels over the two), a
 * mixed batch both (a kernel whose class is absent exits at once).  1 forces the one-substream kernel for
 * the whole batch (a two-substream stream is then reported as DVDA_ST_ENVELOPE); 2 = 3.
 * Under 0 a SMALL batch -- at most 4 096 segments and 32 768 access units, counted on the device by the index --
 * is decoded by the wave-cooperative kernel instead (csrc/mlp_coop.h: one wave per (segment, substream), the
 * bit-serial symbol scan in scalar registers, residuals / filter / rematrix at the width they have): BASELINE
 * configs[3]'s 1 024 single access units, a single title, a streaming-tier packet.  64 forces that kernel for any
 * batch; 1 / 2 never use it; 3 = the lane kernels picked per batch as under 0, never the cooperative kernel (tests
 * and soaks that want the lane kernels on small batches). */
int dvda_mlp_hip_set_lanes_per_segment(dvda_mlp_hip_ctx *ctx, uint32_t lanes);

/* Which form the chain passes behind the parse pass take (segments that continue the FIR history of the one before
 * them, src/mlp.c:297-304, 1302; csrc/mlp_chain.h).  0 (default): chosen per batch -- few deferred segments (one title,
 * a small batch): the recursion in place on the planes and a parallel rematrix pass behind it; many: ONE walk over
 * the planes by two-wave workgroups (k_chain_fused).  1 / 2 force the fused / the two-pass form (tests).  Same PCM. */
int dvda_mlp_hip_set_chain_form(dvda_mlp_hip_ctx *ctx, uint32_t form);

/* Per-segment results of the last decode (blocks on `stream`). */
typedef struct dvda_mlp_segment_info {
    uint64_t offset, end;     /* byte range of the segment in the input buffer */
    uint32_t stream, mlp_frames, pcm_frames, status;
} dvda_mlp_segment_info;
int dvda_mlp_hip_segment_info(dvda_mlp_hip_ctx *ctx, uint32_t segment, dvda_mlp_segment_info *info,
                              void *stream);

/* FIR history (reference struct filter_parameters.state, src/mlp.c:73-77, never cleared there)
 * at the END of `segment`, for both substreams: host_fir[2][48] = [substream][channel slot * 8 + tap],
 * tap 0 = most recent output.  Blocks on `stream`. */
int dvda_mlp_hip_segment_fir(dvda_mlp_hip_ctx *ctx, uint32_t segment, int32_t *host_fir, void *stream);

/* FIR history the streams START with (device pointer, [n_streams][2][48], or NULL = fresh
 * decoders).  Lets a caller decode a stream in pieces cut at major syncs. */
int dvda_mlp_hip_set_initial_fir(dvda_mlp_hip_ctx *ctx, const int32_t *d_init_fir);

const char *dvda_mlp_hip_version(void);

/* Self-test: runs the kernels' arithmetic code-book decode on the device for every (book 0..3,
 * 9-bit peek) and returns host_out[book * 512 + peek] = value | length << 8 (value 0xFF = invalid
 * code; book 0 = no code = 0).  The tables it must equal are reference src/mlp_codebook{1,2,3}.json. */
int dvda_mlp_hip_selftest_huff(int device, uint32_t *host_out);

/* Self-test: reads n fields from host_bytes with the kernels' MSB-first bit reader on the device --
 * widths[i] > 0: unsigned field of that many bits (0..32), < 0: signed field of -widths[i] bits (sign bit
 * first, two's complement), 0: nothing -- into host_out[i].  resident != 0 takes the unsigned fields
 * (< 32 bits) through the row loop's branch-free read.  The contract is reference
 * src/bitstream.c:1077-1111, 1198-1206; its known answers are src/bitstream.c:4864-4868, 4940-4944. */
int dvda_mlp_hip_selftest_bits(int device, const uint8_t *host_bytes, uint32_t n_bytes, const int32_t *host_widths,
                               uint32_t n, int64_t *host_out, uint32_t resident);

/* ------------------------------------------------------------------ PCM tier */
/* Raw-PCM AOB tracks: what reference src/dvd-audio.c:1016-1084 (decode_pcm_audio),
 * src/packet.c:61-188 (pack header / PES walk) and src/pcm.c:99-193 (AOB byte un-swizzle, sign
 * extension) do packet by packet, for n_sectors 2048-byte sectors resident in HBM at once.
 * Output: planar int32, channel c at d_pcm[c * stride + frame] -- the order the reference
 * appends into `samples`.  Only whole 2-frame chunks of a packet are decoded (src/pcm.c:149).
 * d_work: device scratch of dvda_pcm_hip_workspace_words(n_sectors) uint32 words.  After the call
 * it holds, per sector, what the sector contributed and where it starts in the output:
 *   d_work[s]                 PCM frames (or MLP payload bytes, for the demux call) of sector s
 *   d_work[n_sectors + s]     their exclusive prefix sum; d_work[2 * n_sectors] = the total
 * (the disc tier reads the prefix to cut a track at a sector boundary).
 * stride must hold every PCM frame the sectors can contain -- at most n_sectors * 2 * (2048 / chunk bytes): the kernel
 * does not clamp, a sector's frames are written wherever the counts before it put them.  d_pcm may have any 4-byte
 * alignment and stride any parity (8-byte stores where d_pcm is 8-byte aligned and stride even, 4-byte stores
 * otherwise: the same planes); d_sectors must be 16-byte aligned.  Values behind a channel's frames are not written. */
size_t dvda_pcm_hip_workspace_words(uint32_t n_sectors);
int dvda_pcm_hip_decode_sectors(const uint8_t *d_sectors, uint32_t n_sectors, unsigned bits_per_sample,
                                unsigned channels, int32_t *d_pcm, uint64_t stride, uint32_t *d_work,
                                void *stream);
/* blocks on `stream`; *bad_sectors = sectors whose pack / PES / codec header was malformed */
int dvda_pcm_hip_result(const uint32_t *d_work, uint32_t n_sectors, uint64_t *pcm_frames,
                        uint32_t *bad_sectors, void *stream);

/* MLP track demux: AOB sectors of an MLP track -> the contiguous MLP byte
 * stream (every 0xBD packet with codec 0xA1, audio header and pad_2 stripped, in order: what
 * reference src/dvd-audio.c:1151-1227 enqueues packet by packet).  d_work as for the PCM tier;
 * dvda_pcm_hip_result() then returns the byte count in *pcm_frames and the malformed sectors.
 * d_mlp must be 4-byte aligned.  mlp_cap may be smaller than the payload and need not be a multiple of 4: no byte at
 * or behind it is written, every byte below the last whole dword under it (offsets < (mlp_cap & ~3)) is, the 1-3 bytes
 * between may be left untouched (a dword that straddles the cap is dropped whole), and the byte count reported is
 * still the full one. */
int dvda_mlp_hip_demux_sectors(const uint8_t *d_sectors, uint32_t n_sectors, uint8_t *d_mlp,
                               uint64_t mlp_cap, uint32_t *d_work, void *stream);

/* Output stage: planar int32 PCM -> the interleaved little-endian WAV payload
 * dvda2wav writes: frame-major interleave of reference src/dvd-audio.c:781-792, each value as
 * write_signed(bits) (utils/dvda2wav.c:326-334, src/bitstream.c:2846-2857).  bits = 16 or 24;
 * d_out receives frames * channels * bits/8 bytes and not one more.  d_pcm may have any 4-byte alignment, d_out any
 * byte alignment, stride any value >= frames (only the first `frames` values of a plane are read): 16-byte aligned
 * planes (d_pcm and stride * 4) with a 4-byte aligned d_out take the fast kernel for whole 1024-frame blocks, anything
 * else the generic one -- the same bytes. */
int dvda_mlp_hip_pack_wav(const int32_t *d_pcm, uint64_t stride, unsigned channels, uint64_t frames,
                          unsigned bits_per_sample, uint8_t *d_out, void *stream);

/* ------------------------------------------------------------------ digest of the decoded PCM
 * A CRC-32 per stream, computed on the device from whichever layout the decode wrote, so that a caller who only
 * verifies -- an archive against stored checksums, two rips of one disc, new kernels against recorded results --
 * copies 4 bytes per stream to the host and not the payload (csrc/pcm_digest.h).
 *
 * The contract.  For one stream of `frames` PCM frames with `channels` channels at `bits` = 16 or 24, the payload is
 * the byte string dvda2wav writes as the WAV data chunk: frames ascending, the channels of a frame in RIFF-WAVE order,
 * every value v as bits / 8 little-endian bytes of (v & (2^(bits-1) - 1)) | (v < 0 ? 2^(bits-1) : 0) -- write_signed,
 * exactly what dvda_mlp_hip_pack_wav and DVDA_PCM_WAV24 / WAV16 produce.  The digest is zlib's crc32 of that string:
 * reflected polynomial 0xEDB88320, 0xFFFFFFFF as initial value and as final XOR; an empty payload gives 0.  It is the
 * same number whichever of the four DVDA_PCM_* layouts the samples sit in.
 *
 * The kernels cut a payload into tiles of DVDA_CRC_TILE_BYTES, aligned to the payload's END (the first tile of a stream
 * is the ragged one), and one workgroup joins a stream's tiles DVDA_CRC_JOIN_TILES per turn of its loop. */
#define DVDA_CRC_TILE_BYTES  16384u
#define DVDA_CRC_JOIN_TILES  256u

/* where a stream lies in d_pcm: as d_out_off[i] / d_out_stride[i] of dvda_mlp_hip_decode say it, with the PCM frames
 * and channels it holds.  channels outside 1..8 or frames above 2^40: an empty stream. */
typedef struct dvda_pcm_crc_desc {
    uint64_t off;         /* int32 units from d_pcm (WAV layouts: the payload starts at byte 4 * off)   */
    uint64_t stride;      /* capacity in PCM frames (planar: distance between the channels' planes)    */
    uint64_t frames;      /* PCM frames the digest covers; values behind them are not read              */
    uint32_t channels;
    uint32_t reserved;
} dvda_pcm_crc_desc;

/* The tier-free form: d_crc[i], d_nbytes[i] = digest and payload bytes of stream d_desc[i] (device arrays, n entries),
 * from d_pcm in `layout` (DVDA_PCM_*).  Enqueued on `stream`: no host wait, no allocation.  max_total_bytes: a bound the
 * host knows on the sum of the streams' payload bytes -- the launch and d_work are sized by it; a stream whose tiles
 * fall outside it is reported as (0, 0), never read out of bounds.  d_work: dvda_pcm_hip_crc32_workspace_words(n,
 * max_total_bytes) uint32 words, which need not be cleared between calls.  In the WAV layouts a stream's last, partly
 * filled dword is read whole, and no word behind it.  The arguments are judged first, on any machine -- DVDA_HIP_EINVAL:
 * bits other than 16 / 24, a WAV layout of the other depth, a null pointer, work_words too small; DVDA_HIP_ECAPACITY:
 * 2^31 tiles or more -- then the device: DVDA_HIP_ENODEV without one (asked of the runtime once per process). */
size_t dvda_pcm_hip_crc32_workspace_words(uint32_t n, uint64_t max_total_bytes);
int dvda_pcm_hip_crc32(const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc, uint32_t n,
                       uint64_t max_total_bytes, uint32_t *d_crc, uint64_t *d_nbytes, uint32_t *d_work,
                       size_t work_words, void *stream);

/* The convenience call behind dvda_mlp_hip_decode (blocks): host_crc[i], host_nbytes[i] for the first n streams of the
 * last decode, d_pcm / d_out_off / d_out_stride as that decode got them, in the context's layout.  Frames and channels
 * are what dvda_mlp_hip_stream_info reports, so conceal mode's composed stream and the presentation's k channels count
 * as they are; a stream that carries DVDA_ST_OVERFLOW gives (0, 0) -- its region does not hold it -- and every other
 * stream digests the pcm_frames it reports.  The workspace belongs to the context and only grows. */
int dvda_mlp_hip_pcm_crc32(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off,
                           const uint64_t *d_out_stride, unsigned bits, uint32_t *host_crc, uint64_t *host_nbytes,
                           uint32_t n, void *stream);

/* crc(A || B) from crc(A), crc(B) and B's length: how a caller joins pieces -- windows of a track, parts of a title
 * decoded in several batches.  Host arithmetic; needs no device. */
uint32_t dvda_pcm_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ------------------------------------------------------------------ level report of the decoded PCM
 * The digest's sibling: what a caller who verifies a rip asks of the PCM besides "is it the same" -- did the WAV payload
 * wrap, what is the peak of each channel, how much digital silence opens and closes the stream -- answered on the
 * device from the int32 PCM where the decode wrote it (csrc/pcm_levels.h).  The decode clamps
 * nothing to the nominal bit depth; write_signed, dvda_mlp_hip_pack_wav, DVDA_PCM_WAV24 / WAV16 and the digest all take a
 * value modulo 2^bits, so a value outside the nominal range -- a damaged or concealed track can produce one -- is written
 * as a different sample: `over` counts those.
 *
 * The contract.  For one stream of `frames` PCM frames with `channels` channels at nominal depth `bits` = 16, 20 or 24,
 * channels in RIFF-WAVE order as they lie in the buffer, every figure exact.  An all-zero stream has lead_silent ==
 * trail_silent == frames; frames == 0 gives a zeroed struct; entries at index `channels` and above are 0.  The report is
 * the same for DVDA_PCM_PLANAR and DVDA_PCM_INTERLEAVED.  The WAV layouts are DVDA_HIP_EINVAL: their values are already
 * wrapped, the report would say nothing.
 *
 * The kernels cut a stream into tiles of DVDA_LVL_TILE_FRAMES frames, aligned to the stream's START (the last tile is
 * the ragged one).
 *
 * Out of scope: dvda2wav_hip (its readers are WAV-payload readers), the streaming tier, dvda_mlp_hip_decode_multi,
 * reports from the WAV layouts.  RMS and peak over time are the energy report's (below: sums of squares as 128 bits);
 * K-weighted loudness stays out there too. */
#define DVDA_LVL_TILE_FRAMES 4096u

typedef struct dvda_pcm_levels {
    uint64_t frames;          /* PCM frames covered */
    uint64_t lead_silent;     /* frames from the start in which every channel is 0 */
    uint64_t trail_silent;    /* frames up to the end in which every channel is 0 */
    int64_t  sum[8];          /* exact sum of the channel's values */
    uint64_t over[8];         /* values outside [-2^(bits-1), 2^(bits-1) - 1] */
    int32_t  min[8], max[8];  /* smallest / largest value of the channel */
} dvda_pcm_levels;

/* The tier-free form: d_levels[i] = the report of stream d_desc[i] (device arrays, n entries; the digest's descriptor,
 * unchanged: off, stride, frames, channels -- channels outside 1..8 or frames above 2^40: an empty stream), from d_pcm in
 * `layout` (DVDA_PCM_PLANAR or DVDA_PCM_INTERLEAVED).  Enqueued on `stream`: no host wait, no allocation.
 * max_total_frames: a bound the host knows on the sum of the streams' frames -- the launch and d_work are sized by it; a
 * stream whose tiles fall outside it is reported as zeros (frames == 0 too), never read out of bounds.  d_work:
 * dvda_pcm_hip_levels_workspace_words(n, max_total_frames) uint32 words, which need not be cleared between calls; the
 * report is the same from run to run whatever they held (no atomics).  d_pcm + off may have any 4-byte alignment and a
 * planar stride any parity: 16-byte loads wherever memory allows them, the values at a run's ragged ends one by one;
 * nothing outside a stream's `frames` is read.  The arguments are judged first, on any machine -- DVDA_HIP_EINVAL: bits
 * other than 16 / 20 / 24, a WAV layout, a null pointer, work_words too small; DVDA_HIP_ECAPACITY: 2^31 tiles or more --
 * then the device: DVDA_HIP_ENODEV without one (asked of the runtime once per process). */
size_t dvda_pcm_hip_levels_workspace_words(uint32_t n, uint64_t max_total_frames);
int dvda_pcm_hip_levels(const int32_t *d_pcm, uint32_t layout, unsigned bits, const dvda_pcm_crc_desc *d_desc, uint32_t n,
                        uint64_t max_total_frames, dvda_pcm_levels *d_levels, uint32_t *d_work, size_t work_words,
                        void *stream);

/* The convenience call behind dvda_mlp_hip_decode (blocks): host_levels[i] for the first n streams of the last decode,
 * d_pcm / d_out_off / d_out_stride as that decode got them, in the context's layout (DVDA_HIP_EINVAL when that is a WAV
 * one).  Frames and channels are what dvda_mlp_hip_stream_info reports, so conceal mode's composed stream -- its gaps
 * are exact zeros -- and the presentation's k channels count as they are; a stream that carries DVDA_ST_OVERFLOW gives
 * zeros.  The workspace belongs to the context and only grows. */
int dvda_mlp_hip_pcm_levels(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off,
                            const uint64_t *d_out_stride, unsigned bits, dvda_pcm_levels *host_levels, uint32_t n,
                            void *stream);

/* levels(A || B) from levels(A) and levels(B): how a caller joins pieces -- windows of a track, parts of a title.  Lead:
 * a.lead_silent == a.frames ? a.frames + b.lead_silent : a.lead_silent; trail symmetric; an operand with frames == 0 is
 * neutral (its zero min / max do not reach the result).  Either operand may be `out`.  Host arithmetic; needs no device. */
void dvda_pcm_hip_levels_combine(const dvda_pcm_levels *a, const dvda_pcm_levels *b, dvda_pcm_levels *out);

/* ------------------------------------------------------------------ compare of two PCM buffers
 * The third report: when two digests disagree -- two rips of one disc, a concealed track against a good one, a variant
 * build against its parent, the planar against the frame-major instance of a kernel -- where do the two differ, in which
 * channels, and by how much; answered on the device from both int32 buffers where they lie (csrc/pcm_compare.h,
 * DESIGN.md section 14), 160 bytes per stream pair instead of two payloads.  Exact and the same from run to run.
 *
 * The contract.  Two sides, A and B, each with its own buffer, its own layout (DVDA_PCM_PLANAR or DVDA_PCM_INTERLEAVED,
 * chosen per side: all four combinations) and its own descriptor array (the digest's descriptor, unchanged).  Stream i
 * of A is compared with stream i of B over the first `compared` = min(frames_a, frames_b) frames; frames at and behind
 * `compared` on the longer side are not read, and nothing outside a stream's `frames` is read on either side.
 *   bits == 0           the values are compared as the int32 they are; |a - b| is taken in 64 bits, so it is at most
 *                       2^32 - 1 and fits max_abs
 *   bits == 16, 20, 24  each value is first taken as it would be written: w(v) = (v & (2^(bits-1) - 1)) -
 *                       (v < 0 ? 2^(bits-1) : 0), write_signed(bits) read back -- the digest's rule, not plain
 *                       truncation; two values that give the same WAV sample are equal, |w(a) - w(b)| is the difference
 *   any other bits      DVDA_HIP_EINVAL
 * Entries at index `channels` and above are 0.  The result is the same for every combination of layouts, for any 4-byte
 * alignment of either side's `off` independently of the other's, and for any parity of a planar stride.
 *
 * The kernels cut a pair into tiles of DVDA_CMP_TILE_FRAMES frames, aligned to the streams' START.
 *
 * Out of scope: the WAV layouts (DVDA_HIP_EINVAL on either side), the disc tier (its readers keep PCM on the host once
 * they are open, and windowed readers' windows do not line up between two discs), the streaming tier and
 * dvda_mlp_hip_decode_multi, a search for a lag between the sides (a caller shifts off / frames in a descriptor), a merge
 * that fills one rip's concealed spans from another (this report is its first step). */
#define DVDA_CMP_TILE_FRAMES 4096u
#define DVDA_CMP_SHAPE 1u          /* flags: nothing was compared: the channel counts differ, or a descriptor
                                      is one the reports do not take (channels outside 1..8, frames > 2^40) */
typedef struct dvda_pcm_diff {
    uint64_t frames_a, frames_b;   /* as the descriptors say (0 for a descriptor that is not taken) */
    uint64_t compared;             /* min(frames_a, frames_b); 0 with DVDA_CMP_SHAPE */
    uint64_t diff_frames;          /* frames f < compared in which at least one channel differs */
    uint64_t first_diff;           /* the smallest such f; == compared when there is none */
    uint64_t diff_end;             /* the largest such f, + 1; 0 when there is none */
    uint64_t runs;                 /* maximal runs of consecutive differing frames */
    uint64_t diff_values[8];       /* per channel (RIFF-WAVE order, as in the buffers): values that differ */
    uint32_t max_abs[8];           /* per channel: the largest |a - b| */
    uint32_t channels, flags;      /* the pair's channel count (0 with DVDA_CMP_SHAPE); DVDA_CMP_* */
} dvda_pcm_diff;                   /* 160 bytes */

/* The tier-free form: d_diff[i] = the comparison of stream d_desc_a[i] of d_a (in layout_a) with stream d_desc_b[i] of
 * d_b (in layout_b); device arrays, n entries each.  Enqueued on `stream`: no host wait, no allocation.
 * max_total_frames: a bound the host knows on the sum of `compared` over all pairs -- the launch and d_work are sized by
 * it; a pair whose tiles fall outside it is reported as a zeroed struct, never read out of bounds.  d_work:
 * dvda_pcm_hip_compare_workspace_words(n, max_total_frames) uint32 words, which need not be cleared between calls (no
 * atomics: every word the join reads was stored by the same call).  The arguments are judged first, on any machine --
 * DVDA_HIP_EINVAL: bits other than 0 / 16 / 20 / 24, a WAV layout on either side, a null pointer, work_words too small;
 * DVDA_HIP_ECAPACITY: 2^31 tiles or more -- then the device: DVDA_HIP_ENODEV without one. */
size_t dvda_pcm_hip_compare_workspace_words(uint32_t n, uint64_t max_total_frames);
int dvda_pcm_hip_compare(const int32_t *d_a, uint32_t layout_a, const dvda_pcm_crc_desc *d_desc_a,
                         const int32_t *d_b, uint32_t layout_b, const dvda_pcm_crc_desc *d_desc_b,
                         uint32_t n, unsigned bits, uint64_t max_total_frames, dvda_pcm_diff *d_diff,
                         uint32_t *d_work, size_t work_words, void *stream);
/* behind dvda_mlp_hip_decode (blocks): side A = the first n streams of the context's last decode, frames and
 * channels as dvda_mlp_hip_stream_info reports them (conceal mode's composed stream and the presentation count as
 * they are; a stream with DVDA_ST_OVERFLOW is an empty side); side B = the caller's buffer, layout and DEVICE
 * descriptor array.  DVDA_HIP_EINVAL on a context that writes a WAV layout. */
int dvda_mlp_hip_pcm_compare(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off,
                             const uint64_t *d_out_stride, const int32_t *d_other, uint32_t other_layout,
                             const dvda_pcm_crc_desc *d_other_desc, unsigned bits, dvda_pcm_diff *host_diff,
                             uint32_t n, void *stream);
/* diff(A1 || A2, B1 || B2) from the diffs of the two pieces; host arithmetic, no device; either operand may be out.
 * An operand with frames_a == frames_b == 0 and no flag is neutral.  Otherwise DVDA_HIP_EINVAL, `out` left alone, when
 * the first operand has frames_a != frames_b (the pieces would not line up), when the operands' channel counts differ,
 * or when either carries DVDA_CMP_SHAPE.  Counts add, max_abs is the maximum, first_diff / diff_end move by a.compared,
 * and a run that crosses the seam counts once. */
int dvda_pcm_hip_diff_combine(const dvda_pcm_diff *a, const dvda_pcm_diff *b, dvda_pcm_diff *out);

/* ------------------------------------------------------------------ energy report of the decoded PCM
 * The fourth report: what a ripper or an archive computes from every sample over time -- the RMS level of a track, its
 * crest factor, the block statistics a dynamic-range meter works from, the min / max envelope a GUI draws -- comes from
 * two figures per block of frames and channel: the sum of v * v and the largest |v|.  They are computed on the device
 * from the int32 PCM where the decode wrote it (csrc/pcm_energy.h), 168 bytes per block instead
 * of the payload.  A square of an int32 is at most 2^62 and a stream has at most 2^40 frames, so a sum is below 2^102:
 * two 64-bit words hold it exactly.  Integer arithmetic throughout: the same words in any order, from either layout,
 * from run to run.
 *
 * The contract.  One stream of `frames` PCM frames with `channels` channels, int32 PCM in DVDA_PCM_PLANAR or
 * DVDA_PCM_INTERLEAVED, channels as they lie in the buffer, values as they are: nothing is clamped, there is no `bits`.
 * The block grid: a block length `block_frames` = B in DVDA_NRG_MIN_BLOCK .. DVDA_NRG_MAX_BLOCK (otherwise
 * DVDA_HIP_EINVAL) and, per stream, the length `lead` in 1 .. B of the first block (a NULL array: B for every stream; a
 * lead outside 1 .. B: the stream has no blocks).  Frame f lies in block 0 when f < lead, else in block
 * 1 + (f - lead) / B; nblocks = 0 for no frames, else 1 + ceil(max(frames - lead, 0) / B).  `lead` is there so that a
 * piece of a longer track -- a window -- can sit on the track's grid.  Entries at index `channels` and above are 0.  A
 * descriptor the other reports do not take (channels outside 1..8, frames above 2^40) has no blocks.  The two int32
 * layouts give the same report; the WAV layouts are DVDA_HIP_EINVAL, as for the level report.
 *
 * The kernels cut a block into pieces of at most DVDA_NRG_PIECE_FRAMES frames, one workgroup per piece.
 *
 * What a caller derives from these integers -- RMS in dBFS, crest factor, a DR figure, an overview -- is host
 * arithmetic of the caller's.  Out of scope: K-weighted loudness (BS.1770: floating-point filtering, it cannot be
 * exact), dvda2wav_hip, the streaming tier, dvda_mlp_hip_decode_multi, reports from the WAV layouts. */
#define DVDA_NRG_MIN_BLOCK    64u
#define DVDA_NRG_MAX_BLOCK    16777216u
#define DVDA_NRG_PIECE_FRAMES 4096u

typedef struct dvda_pcm_energy_block {   /* 168 bytes */
    uint64_t sq_lo[8], sq_hi[8];  /* sum of v*v of the channel over the block = sq_hi * 2^64 + sq_lo, exact   */
    uint32_t peak[8];             /* largest |v| of the channel in the block (2^31 for v = -2^31)             */
    uint32_t frames;              /* frames the block holds: B, fewer in a first block (lead) and in the last */
    uint32_t reserved;            /* 0 */
} dvda_pcm_energy_block;

/* The tier-free form.  Stream i (descriptor d_desc[i], first block d_lead[i] frames; device arrays, n entries) leaves
 * its records in d_blocks[d_block_off[i] + j] for j < d_block_cap[i], and in d_nblocks[i] how many blocks it has: more
 * than its cap means that only cap were written, and nothing was written behind them.  Enqueued on `stream`: no host
 * wait, no allocation.  max_total_frames: a bound the host knows on the sum of the streams' frames -- the launch and
 * d_work are sized by it (at most max_total_frames / DVDA_NRG_PIECE_FRAMES + max_total_frames / B + 2 n pieces); a
 * stream whose pieces fall outside it reports 0 blocks and is never read out of bounds.  d_work:
 * dvda_pcm_hip_energy_workspace_words(n, max_total_frames, block_frames) uint32 words (0 for a block_frames outside its
 * range), which need not be cleared between calls; no atomics, the words are the same from run to run.  d_pcm + off may
 * have any 4-byte alignment and a planar stride any parity; nothing outside a stream's `frames` is read.  The arguments
 * are judged first, on any machine -- DVDA_HIP_EINVAL: block_frames outside its range, a WAV layout, a null pointer
 * other than d_lead, work_words too small; DVDA_HIP_ECAPACITY: 2^31 pieces or more -- then the device: DVDA_HIP_ENODEV
 * without one. */
size_t dvda_pcm_hip_energy_workspace_words(uint32_t n, uint64_t max_total_frames, uint32_t block_frames);
int dvda_pcm_hip_energy(const int32_t *d_pcm, uint32_t layout, const dvda_pcm_crc_desc *d_desc, uint32_t n,
                        uint32_t block_frames, const uint32_t *d_lead /* or NULL */, uint64_t max_total_frames,
                        dvda_pcm_energy_block *d_blocks, const uint64_t *d_block_off, const uint64_t *d_block_cap,
                        uint64_t *d_nblocks, uint32_t *d_work, size_t work_words, void *stream);

/* behind dvda_mlp_hip_decode (blocks): the blocks of the first n streams of the last decode, every stream's grid
 * starting at its first frame (lead = B).  Frames and channels are what dvda_mlp_hip_stream_info reports: conceal
 * mode's composed stream and the presentation's k channels count as they are; a stream that carries DVDA_ST_OVERFLOW
 * has no blocks.  The streams lie back to back in host_blocks, stream i in [host_first[i], host_first[i + 1]).  When
 * cap_blocks is too small: DVDA_HIP_ECAPACITY with host_first[n] = the count needed and nothing else written.
 * DVDA_HIP_EINVAL on a context that writes a WAV layout.  The workspace belongs to the context and only grows. */
int dvda_mlp_hip_pcm_energy(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off,
                            const uint64_t *d_out_stride, uint32_t block_frames, dvda_pcm_energy_block *host_blocks,
                            uint64_t cap_blocks, uint64_t *host_first /* [n + 1] */, uint32_t n, void *stream);

/* Host arithmetic; needs no device.
 * append: joins a piece's blocks to a track's (*n_track blocks in track[0, cap), a grid that starts at the track's first
 * frame).  When the track's last block is short (frames < B) the piece's first block is added into it -- 128-bit add
 * with carry, the larger peak, frames added -- and a sum of frames above B is DVDA_HIP_EINVAL: the piece was not on the
 * grid (so is a sum below B with more blocks behind it, and a short block inside the piece).  The rest of the piece is
 * appended.  DVDA_HIP_ECAPACITY when cap does not hold the result.  On an error nothing
 * is written.  `piece` must not overlap `track`.  The lead of the next piece is B - (frames so far mod B).
 * total: folds n blocks into one record: sums added, the largest peak; its `frames` field saturates at 2^32 - 1. */
int dvda_pcm_hip_energy_append(dvda_pcm_energy_block *track, uint64_t *n_track, uint64_t cap,
                               const dvda_pcm_energy_block *piece, uint64_t n_piece, uint32_t block_frames);
void dvda_pcm_hip_energy_total(const dvda_pcm_energy_block *blocks, uint64_t n, dvda_pcm_energy_block *out);

/* ------------------------------------------------------------------ word-length reduction of the decoded PCM
 * The first pass that writes PCM: a track delivered at a smaller word length -- 24-bit audio as a 16-bit file for a CD, a
 * portable player, a preview -- made on the device while the samples are still there, truncated, rounded or dithered, and
 * CLAMPED to the output range where write_signed would wrap (csrc/pcm_requant.h).  A 16-bit
 * payload is half of what the 24-bit one moves to the host and a third of the int32 PCM.
 *
 * The contract; every figure exact.  s = bits_in - bits_out with bits_in, bits_out in {16, 20, 24} and bits_out <=
 * bits_in, so s is 0, 4 or 8.  For the value v (any int32; the arithmetic as if in 64 bits) of channel c -- its position
 * in the buffer, RIFF-WAVE order -- at absolute frame F = frame0 + f:
 *   DVDA_RQ_TRUNCATE   q = v >> s (arithmetic shift: floor)
 *   DVDA_RQ_ROUND      q = (v + 2^(s-1)) >> s
 *   DVDA_RQ_TPDF       q = (v + 2^(s-1) + u1 - u2) >> s, u1 and u2 two s-bit uniforms: their difference is triangular
 *                      over +-(2^s - 1), +-1 output LSB
 *   s == 0             q = v in every mode: a pure clamp
 * and the output is clamp(q, -2^(bits_out-1), 2^(bits_out-1) - 1); clipped[c] counts the values the clamp changed.
 * The noise is a counter-based function of (seed, F, c), one 64-bit word per FOUR frames of a channel: with Q = F >> 2,
 * j = F & 3, all arithmetic mod 2^64,
 *   z = seed + 0x9E3779B97F4A7C15 * (8 Q + c + 1)
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 *   field = (z >> (16 j)) & 0xFFFF;  u1 = field & (2^s - 1);  u2 = (field >> 8) & (2^s - 1)
 * (z is output number 8 Q + c + 1 of splitmix64 seeded with `seed`).  frame0 is how a caller says "this piece starts at
 * frame N of the track": a track requantized in one piece, in windows or on several devices is the same bytes.  The
 * reports of two pieces join by adding `frames` and clipped[]; there is no combine function.
 *
 * Out of scope: noise shaping (error feedback is a serial nonlinear recurrence per channel), sample-rate conversion
 * (but see the decimation by 2 or 4 and the 48 -> 44.1 kHz resampler below), auto-blanking of digital silence (TPDF on
 * silence is noise of +-1 LSB, as it should be), float output, the streaming tier and dvda_mlp_hip_decode_multi.  The disc tier has it as
 * dvda_hip_set_requantize (dvd-audio-hip.h). */
#define DVDA_RQ_TRUNCATE 0u
#define DVDA_RQ_ROUND    1u
#define DVDA_RQ_TPDF     2u
typedef struct dvda_pcm_requant {
    uint32_t bits_in, bits_out;   /* 16, 20 or 24; bits_out <= bits_in */
    uint32_t mode;                /* DVDA_RQ_* */
    uint32_t reserved;            /* 0 */
    uint64_t seed;                /* of the dither's noise (DVDA_RQ_TPDF) */
} dvda_pcm_requant;               /* 24 bytes */
typedef struct dvda_pcm_requant_report {
    uint64_t frames;              /* PCM frames requantized */
    uint64_t clipped[8];          /* per channel: values the clamp changed */
} dvda_pcm_requant_report;        /* 72 bytes */

/* The tier-free form.  Stream i: d_desc_in[i] in d_in (layout_in: DVDA_PCM_PLANAR or DVDA_PCM_INTERLEAVED) ->
 * d_desc_out[i] in d_out, first absolute frame d_frame0[i] (a NULL array: 0 for every stream), report d_report[i]; device
 * arrays, n entries.  layout_out: either int32 layout for any bits_out -- the values lie in the output range -- or
 * DVDA_PCM_WAV16 when bits_out == 16 / DVDA_PCM_WAV24 when bits_out == 24: the payload exactly as dvda_mlp_hip_pack_wav
 * would write it from the int32 result, from byte 4 * off on, frames * channels * bits_out / 8 bytes and not one more.
 * A stream is not taken -- frames == 0 reported, nothing written -- when its input descriptor is one the reports do not
 * take (channels outside 1..8, frames above 2^40) or its output descriptor has other frames / channels or a stride below
 * its frames.  In place: d_out == d_in with the same int32 layout and the same descriptors is allowed and exact; any
 * other overlap is the caller's error.  Enqueued on `stream`: no host wait, no allocation.  max_total_frames: a bound the
 * host knows on the sum of the streams' frames; a stream whose tiles (DVDA_LVL_TILE_FRAMES frames, aligned to its start)
 * fall outside it reports zeros, and its output region holds unspecified values inside its bounds and nothing outside
 * them.  d_work: dvda_pcm_hip_requantize_workspace_words(n, max_total_frames) uint32 words, which need not be cleared;
 * no atomics, the report is the same from run to run.  Either side's off may have any 4-byte alignment and a planar
 * stride any parity: 16-byte accesses wherever memory allows them; nothing outside a stream's `frames` is read, nothing
 * outside its output region written.  The arguments are judged first, on any machine -- DVDA_HIP_EINVAL: bits outside
 * {16, 20, 24} or bits_out > bits_in, a mode above 2, reserved != 0, a WAV input layout, a WAV output layout of another
 * depth than bits_out (or any for bits_out == 20), a null pointer other than d_frame0, work_words too small;
 * DVDA_HIP_ECAPACITY: 2^31 tiles or more -- then the device: DVDA_HIP_ENODEV without one. */
size_t dvda_pcm_hip_requantize_workspace_words(uint32_t n, uint64_t max_total_frames);
int dvda_pcm_hip_requantize(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                            int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                            const uint64_t *d_frame0 /* or NULL */, uint32_t n, const dvda_pcm_requant *params /* host */,
                            uint64_t max_total_frames, dvda_pcm_requant_report *d_report,
                            uint32_t *d_work, size_t work_words, void *stream);

/* behind dvda_mlp_hip_decode (blocks): the first n streams of the last decode requantized IN PLACE, d_pcm / d_out_off /
 * d_out_stride as that decode got them, in the context's layout (DVDA_HIP_EINVAL when that is a WAV one); stream i starts
 * at absolute frame host_frame0[i] (NULL: 0).  Frames and channels are what dvda_mlp_hip_stream_info reports; a stream
 * that carries DVDA_ST_OVERFLOW is untouched and reports zeros.  Behind it dvda_mlp_hip_pcm_crc32(ctx, ..., bits_out),
 * dvda_mlp_hip_pcm_levels and dvda_mlp_hip_pcm_energy see the requantized PCM. */
int dvda_mlp_hip_pcm_requantize(dvda_mlp_hip_ctx *ctx, int32_t *d_pcm, const uint64_t *d_out_off, const uint64_t *d_out_stride,
                                const dvda_pcm_requant *params, const uint64_t *host_frame0 /* or NULL */,
                                dvda_pcm_requant_report *host_report, uint32_t n, void *stream);

/* The contract above for one value: host arithmetic, needs no device -- the text the kernel compiles.  `frame` is the
 * absolute frame.  *clipped (may be NULL) = 1 when the clamp changed the value, else 0; invalid params: returns 0 and
 * sets *clipped = -1. */
int32_t dvda_pcm_hip_requant_value(int32_t v, uint64_t frame, uint32_t channel, const dvda_pcm_requant *params, int *clipped);

/* ------------------------------------------------------------------ decimation of the decoded PCM by 2 or 4
 * DVD-Audio tracks run at 88.2 / 96 / 176.4 / 192 kHz; the file a CD, a player or a preview wants runs at 44.1 or 48 kHz,
 * an integer reduction by 2 or 4 inside the format's two rate families.  Made on the device, the caller does not copy
 * 4 bytes per sample at the high rate to the host in order to throw three quarters of them away (csrc/pcm_decim.h,
 * DESIGN.md section 17).
 *
 * The contract; every figure exact.  Ratio D in {2, 4}.  One tap table per ratio, h_D[0 .. N_D - 1], int32, a committed
 * constant (csrc/pcm_decim_taps.h; dvda_pcm_hip_decim_taps hands it out): N_2 = 191, N_4 = 383, H_D = (N_D - 1) / 2 = 95 /
 * 191; symmetric, h[i] == h[N-1-i]; Q = 30 and sum h = 2^30 exactly, so the gain at DC is exactly 1; every tap at an
 * offset from the centre that is a non-zero multiple of D is exactly 0 (a half-band / quarter-band filter).  Recipe of
 * tools/make_decim_taps.py: 2 fc sinc(2 fc n) * kaiser(N, 12.0), fc = 0.5 / D, normalised, rint(h * 2^30), the sum's
 * difference from 2^30 added to the centre tap -- but the library's truth is the committed integers.  sum |h| =
 * 2 122 621 608 (D = 2) and 2 352 308 816 (D = 4); passband 0 .. 0.4535 fs_out within +-1.2e-5 dB, stopband from
 * 0.5465 fs_out to the input Nyquist at -118.7 dB / -119.2 dB.  With sum |h| < 2.4e9 and |x| <= 2^31 the accumulator
 * stays below 5.2e18 < 2^63 for ANY int32 input: the arithmetic is plain int64 and cannot overflow.
 *
 * For channel c and output frame M (absolute, on the track's grid), x[F][c] the input at absolute frame F:
 *   acc     = sum_{k = -H .. H} h[H + k] * x[D M + k][c]                                   (int64)
 *   y[M][c] = clamp((acc + 2^29) >> 30, -2^(bits-1), 2^(bits-1) - 1)     bits in {16, 20, 24}; the shift is arithmetic
 * x[F] = 0 wherever the region does not hold F: in front of the track's first frame, behind its last one, beyond the
 * context a piece brought.  clipped[c] counts the values the clamp changed (a band-limited version of full-scale
 * material overshoots).  A track of F frames gives ceil(F / D) frames, M = 0 .. ceil(F / D) - 1.
 *
 * Pieces.  A stream may be a piece of a track: of the input descriptor's `frames` = before + own + after, the first
 * `before` and the last `after` frames are context -- read, nothing produced for them -- and the own frames in between are
 * the track's absolute frames [frame0, frame0 + own).  The piece's outputs are the M with frame0 <= D M < frame0 + own:
 * dvda_pcm_hip_decim_out_frames(frame0, own, ratio) = ceil((frame0 + own) / D) - ceil(frame0 / D) of them (a host
 * function; the kernels ask the same one; 0 for another ratio or frame0 / own above 2^62).  Only the H context frames
 * nearest the own frames matter.  A piece whose context on each side is at least H frames, or reaches the track's end on
 * that side, gives exactly the frames the whole track gives at those M; the reports of two pieces join by adding, there
 * is no combine function.  d_piece == NULL: whole tracks, frame0 = 0, no context.  before + after > frames (or frame0
 * above 2^62): the stream is not taken.
 *
 * Out of scope: upsampling, noise shaping, the WAV layouts on either side (requantize behind it writes them), in place,
 * the streaming tier and dvda_mlp_hip_decode_multi.  Between the rate families there is one step, 48 -> 44.1 kHz:
 * dvda_pcm_hip_resample below (96 -> 44.1 is this pass by 2, then that one).  The disc tier has it for tracks read whole:
 * dvda_hip_set_decimate in dvd-audio-hip.h. */
#define DVDA_DCM_TILE_FRAMES 1024u      /* OUTPUT frames of a tile; tiles are aligned to the stream's first output frame */
typedef struct dvda_pcm_decim_piece {
    uint64_t frame0;              /* absolute frame of the first own frame */
    uint32_t before, after;       /* context frames in front of / behind the own frames */
} dvda_pcm_decim_piece;           /* 16 bytes */
typedef struct dvda_pcm_decim_report {
    uint64_t frames_in;           /* own input frames */
    uint64_t frames_out;          /* frames written */
    uint64_t clipped[8];          /* per channel: values the clamp changed */
} dvda_pcm_decim_report;          /* 80 bytes */

/* The tier-free form.  Stream i: d_desc_in[i] in d_in (layout_in) -> d_desc_out[i] in d_out (layout_out), piece d_piece[i]
 * (a NULL array: whole tracks), report d_report[i]; device arrays, n entries; each layout DVDA_PCM_PLANAR or
 * DVDA_PCM_INTERLEAVED.  A stream is taken only when its input descriptor is one the reports take (channels 1..8, frames
 * up to 2^40) and holds its context, and its output descriptor has the same channels, exactly out_frames frames and a
 * stride >= frames; otherwise frames_in == frames_out == 0 is reported and nothing is written.  Out of place only; any
 * overlap is the caller's error.  Enqueued on `stream`: no host wait, no allocation.  max_total_out_frames: a bound the
 * host knows on the sum of the streams' OUTPUT frames; a stream whose tiles (DVDA_DCM_TILE_FRAMES output frames) fall
 * outside it reports zeros, and its output region holds unspecified values inside its bounds and nothing outside them.
 * d_work: dvda_pcm_hip_decimate_workspace_words(n, max_total_out_frames) uint32 words, which need not be cleared; no
 * atomics, the report is the same from run to run.  Either side's off may have any 4-byte alignment and a planar stride
 * any parity: 16-byte loads wherever memory allows them, 16-byte stores to an aligned planar output; nothing outside a
 * region's `frames` is read, nothing outside the output region written.  The arguments are judged first, on any machine
 * -- DVDA_HIP_EINVAL: a ratio other than 2 or 4, bits outside {16, 20, 24}, a WAV layout on either side, a null pointer
 * other than d_piece, work_words too small; DVDA_HIP_ECAPACITY: 2^31 tiles or more -- then the device: DVDA_HIP_ENODEV
 * without one. */
size_t dvda_pcm_hip_decimate_workspace_words(uint32_t n, uint64_t max_total_out_frames);
int dvda_pcm_hip_decimate(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                          int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                          const dvda_pcm_decim_piece *d_piece /* or NULL */, uint32_t n, uint32_t ratio, unsigned bits,
                          uint64_t max_total_out_frames, dvda_pcm_decim_report *d_report,
                          uint32_t *d_work, size_t work_words, void *stream);

/* behind dvda_mlp_hip_decode (blocks): the first n streams of the last decode, whole tracks, d_pcm / d_out_off /
 * d_out_stride as that decode got them, in the context's layout (DVDA_HIP_EINVAL when that is a WAV one), decimated into
 * d_dst (layout_dst: either int32 layout): stream i to the dword offset host_dst_off[i] with the planar stride
 * host_dst_stride[i] (host arrays; a stride below the stream's output frames: the stream is not taken).  Frames and
 * channels are what dvda_mlp_hip_stream_info reports; a stream that carries DVDA_ST_OVERFLOW reports zeros and nothing
 * is written for it. */
int dvda_mlp_hip_pcm_decimate(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off,
                              const uint64_t *d_out_stride, uint32_t ratio, unsigned bits, int32_t *d_dst,
                              uint32_t layout_dst, const uint64_t *host_dst_off, const uint64_t *host_dst_stride,
                              dvda_pcm_decim_report *host_report, uint32_t n, void *stream);

/* Host helpers; none needs a device.  taps: the committed table of `ratio`, *n (may be NULL) = its length; NULL and 0 for
 * another ratio.  value: the contract above for one output value -- the text the kernel compiles -- from its window of
 * 2 H + 1 input values, window[H] the one at D M; *clipped (may be NULL) = 1 when the clamp changed the value, else 0;
 * an invalid ratio or depth or a NULL window: returns 0 and sets *clipped = -1. */
const int32_t *dvda_pcm_hip_decim_taps(uint32_t ratio, uint32_t *n);
uint64_t dvda_pcm_hip_decim_out_frames(uint64_t frame0, uint64_t own, uint32_t ratio);
int32_t dvda_pcm_hip_decim_value(const int32_t *window, uint32_t ratio, unsigned bits, int *clipped);

/* ------------------------------------------------------------------ 48 kHz to 44.1 kHz: the resampler
 * The decimation above stays inside a rate family; a CD runs at 44.1 kHz and most DVD-Audio discs sit in the 48 / 96 /
 * 192 kHz family.  This pass crosses: 48 000 Hz in, 44 100 Hz out, ratio L / M = 147 / 160 and no other (96 / 192 kHz:
 * decimate by 2 / 4 first).  Made on the device (csrc/pcm_resample.h).
 *
 * The contract; every figure exact.  One table g[147][96], int32, Q30, a committed constant (csrc/pcm_resample_taps.h;
 * dvda_pcm_hip_resample_taps hands it out): 147 phases of 96 taps.  Recipe of tools/make_resample_taps.py:
 * h_c(t) = (147/160) sinc((147/160) t) * I0(12 sqrt(1 - (t/48)^2)) / I0(12), t in input samples; g[p][i] =
 * h_c(i - 47 - p/147); every phase normalised to sum 1, rint(. * 2^30), the phase's difference from 2^30 added to that
 * phase's largest tap -- but the library's truth is the committed integers.  Every phase sums to exactly 2^30, so the gain
 * at DC is exactly 1 at every output frame; g[147 - p][i] == g[p][95 - i] for p = 1 .. 146; from an FFT of the integers
 * over the whole 147-times oversampled prototype, images included: passband 0 .. 0.4535 fs_out within +1.2e-5 / -0.9e-5 dB,
 * stopband from 0.5465 fs_out upward at -118.2 dB (the decimator's class); the largest per-phase sum |g| is
 * 2 561 819 644 < 2^32, so with |x| <= 2^31 |acc| + 2^29 < 2^63 for ANY int32 input: the arithmetic is plain int64 and
 * cannot overflow.
 *
 * For channel c and output frame m (absolute, on the track's output grid), x[F][c] the input at absolute frame F:
 *   q       = (160 m) div 147,   p = (160 m) mod 147
 *   acc     = sum_{i = 0 .. 95} g[p][i] * x[q - 47 + i][c]                                (int64)
 *   y[m][c] = clamp((acc + 2^29) >> 30, -2^(bits-1), 2^(bits-1) - 1)     bits in {16, 20, 24}; the shift is arithmetic
 * x[F] = 0 wherever the region does not hold F: in front of the track's first frame, behind its last one, beyond the
 * context a piece brought.  clipped[c] counts the values the clamp changed.  A track of F frames gives ceil(147 F / 160)
 * frames.
 *
 * Pieces: dvda_pcm_decim_piece and dvda_pcm_decim_report as they are above.  A piece's outputs are the m with
 * frame0 <= (160 m) div 147 < frame0 + own: dvda_pcm_hip_resample_out_frames(frame0, own) = ceil(147 (frame0 + own) / 160)
 * - ceil(147 frame0 / 160) of them (a host function; the kernels ask the same one; 0 for frame0 / own above 2^62), and
 * the pieces of a track add up to the track's ceil(147 F / 160).  Only the 47 context frames in front of the own frames
 * and the 48 behind them matter.  A piece whose context on each side is at least 48 frames, or reaches the track's end on
 * that side, gives exactly the frames the whole track gives at those m; the reports of two pieces join by adding.
 * d_piece == NULL: whole tracks, frame0 = 0, no context.  before + after > frames (or frame0 above 2^62): the stream is
 * not taken.
 *
 * Out of scope: any other ratio (upsampling, 44.1 -> 48, 96 -> 44.1 in one step), noise shaping, the WAV layouts on
 * either side (requantize behind it writes them), in place, the streaming tier and dvda_mlp_hip_decode_multi.  The disc
 * tier has it for tracks read whole: dvda_hip_set_resample in dvd-audio-hip.h. */
#define DVDA_RSM_TILE_FRAMES 9408u      /* OUTPUT frames of a tile, 64 * 147; tiles are aligned to the stream's first output frame */

/* The tier-free form, with the decimator's shapes.  Stream i: d_desc_in[i] in d_in (layout_in) -> d_desc_out[i] in d_out
 * (layout_out), piece d_piece[i] (a NULL array: whole tracks), report d_report[i]; device arrays, n entries; each layout
 * DVDA_PCM_PLANAR or DVDA_PCM_INTERLEAVED.  A stream is taken only when its input descriptor is one the reports take
 * (channels 1..8, frames up to 2^40) and holds its context, and its output descriptor has the same channels, exactly
 * out_frames frames and a stride >= frames; otherwise frames_in == frames_out == 0 is reported and nothing is written.
 * Out of place only; any overlap is the caller's error.  Enqueued on `stream`: no host wait, no allocation.
 * max_total_out_frames: a bound the host knows on the sum of the streams' OUTPUT frames; a stream whose tiles
 * (DVDA_RSM_TILE_FRAMES output frames) fall outside it reports zeros, and its output region holds unspecified values
 * inside its bounds and nothing outside them.  d_work: dvda_pcm_hip_resample_workspace_words(n, max_total_out_frames)
 * uint32 words, which need not be cleared; no atomics, the report is the same from run to run.  Either side's off may
 * have any 4-byte alignment and a planar stride any parity; nothing outside a region's `frames` is read, nothing outside
 * the output region written.  The arguments are judged first, on any machine -- DVDA_HIP_EINVAL: bits outside {16, 20,
 * 24}, a WAV layout on either side, a null pointer other than d_piece, work_words too small; DVDA_HIP_ECAPACITY: 2^31
 * tiles or more -- then the device: DVDA_HIP_ENODEV without one. */
size_t dvda_pcm_hip_resample_workspace_words(uint32_t n, uint64_t max_total_out_frames);
int dvda_pcm_hip_resample(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                          int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                          const dvda_pcm_decim_piece *d_piece /* or NULL */, uint32_t n, unsigned bits,
                          uint64_t max_total_out_frames, dvda_pcm_decim_report *d_report,
                          uint32_t *d_work, size_t work_words, void *stream);

/* behind dvda_mlp_hip_decode (blocks): as dvda_mlp_hip_pcm_decimate, the first n streams of the last decode, whole
 * tracks taken as 48 kHz, resampled into d_dst (layout_dst: either int32 layout): stream i to the dword offset
 * host_dst_off[i] with the planar stride host_dst_stride[i] (host arrays; a stride below the stream's output frames: the
 * stream is not taken).  A stream that carries DVDA_ST_OVERFLOW reports zeros and nothing is written for it. */
int dvda_mlp_hip_pcm_resample(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off,
                              const uint64_t *d_out_stride, unsigned bits, int32_t *d_dst, uint32_t layout_dst,
                              const uint64_t *host_dst_off, const uint64_t *host_dst_stride,
                              dvda_pcm_decim_report *host_report, uint32_t n, void *stream);

/* Host helpers; none needs a device.  taps: the committed table, row p at [96 p .. 96 p + 95]; *phases / *taps (either
 * may be NULL) = 147 / 96.  value: the contract above for one output value -- the text the kernel compiles -- from its
 * window of 96 input values, window[47] the one at q, and its phase p; *clipped (may be NULL) = 1 when the clamp changed
 * the value, else 0; a phase above 146, an invalid depth or a NULL window: returns 0 and sets *clipped = -1. */
const int32_t *dvda_pcm_hip_resample_taps(uint32_t *phases, uint32_t *taps);
uint64_t dvda_pcm_hip_resample_out_frames(uint64_t frame0, uint64_t own);
int32_t dvda_pcm_hip_resample_value(const int32_t *window, uint32_t phase, unsigned bits, int *clipped);

/* ------------------------------------------------------------------ channel mix: multichannel PCM to stereo or mono
 * The passes above make a 24-bit 96 kHz track a 16-bit 44.1 kHz one; the file a CD, a portable player or a preview
 * takes has two channels as well, and a one-substream multichannel MLP title or a raw-PCM multichannel track carries no
 * stereo mix of its own (dvda_mlp_hip_set_presentation covers only titles that do).  This pass folds the channels on
 * the device (csrc/pcm_mix.h): out_channels rows of Q30 coefficients over in_channels inputs.  It
 * is the first pass whose output has another channel count than its input.
 *
 * The contract; every figure exact.  For frame f and output channel o, x[f][c] ANY int32, channels in RIFF-WAVE order
 * as they lie in the buffer:
 *   acc     = sum_{c < in_channels} coef[o][c] * x[f][c]                                   (int64)
 *   y[f][o] = clamp((acc + 2^29) >> 30, -2^(bits-1), 2^(bits-1) - 1)     bits in {16, 20, 24}; the shift is arithmetic
 * clipped[o] counts the values the clamp changed.
 *
 * Validity: a matrix is valid when both channel counts lie in 1..8 and every used row has sum_c |coef[o][c]| <= 2^31
 * (c < in_channels; entries outside [out_channels)[in_channels) are ignored).  Then for any int32 input |x| <= 2^31, so
 * |acc| <= sum_c |coef[o][c]| * 2^31 <= 2^62 and |acc + 2^29| <= 2^62 + 2^29 < 2^63: the arithmetic is plain int64 and
 * cannot overflow.  A stream whose matrix is invalid, or whose channel counts do not match its descriptors, is not
 * taken: frames == 0 is reported and nothing is written.
 *
 * The pass is pointwise in the frame: a track mixed whole, in pieces or on several devices gives the same bytes, with
 * no context frames, and the reports of pieces join by adding their fields.  With 2^30 on the diagonal the output is
 * the input for values inside `bits`; rows can also express a permutation or the extraction of one channel.
 *
 * The default matrices (dvda_pcm_hip_mix_matrix) are Q30 integers: ONE = 2^30, A = 759250125 = rint(2^30 / sqrt 2),
 * HALF = 2^29.  Stereo rows (L, R): FL -> L: ONE; FR -> R: ONE; FC -> both: A; BL -> L: A; BR -> R: A; BC -> both: HALF;
 * LFE -> 0, or both: A with DVDA_MIX_LFE.  The mono row is wL + wR per channel.
 *   DVDA_MIX_NORMALIZED (0, the default): S = the larger of the two row sums (mono: the row's sum), coef = (w << 30) div S
 *     with ONE S for both rows, which keeps the balance.  Input inside `bits` can then never clip: every coef >= 0 and
 *     floor((w << 30) / S) summed over a row is <= (sum w) * 2^30 / S <= 2^30, so with |x| <= 2^(bits-1)
 *     |acc| <= 2^30 * 2^(bits-1); and acc <= 2^30 * (2^(bits-1) - 1) on the positive side, so (acc + 2^29) >> 30 lies in
 *     [-2^(bits-1), 2^(bits-1) - 1].
 *   DVDA_MIX_UNITY: the weights as they are (mono: (wL + wR) >> 1): the fronts at gain 1, and the clamp counts the overs.
 *     Where a row's weights sum above 2^31 -- FL + FC + BL is 2^30 (1 + sqrt 2) -- the matrix made is not a valid one and
 *     a stream given it is not taken: ask dvda_pcm_hip_mix_valid.
 *
 * Out of scope: the disc's own downmix coefficient table (a caller who has it passes it as a dvda_pcm_mix), upmixing
 * rules (though out > in is a valid matrix), float or per-frame gains, dither (requantize behind it dithers), the WAV
 * layouts on either side, in place, the streaming tier and dvda_mlp_hip_decode_multi. */
#define DVDA_MIX_NORMALIZED 0u
#define DVDA_MIX_UNITY      1u
#define DVDA_MIX_LFE        2u

typedef struct dvda_pcm_mix {
    uint32_t in_channels;     /* 1..8; must equal the input descriptor's channels  */
    uint32_t out_channels;    /* 1..8; must equal the output descriptor's channels */
    int32_t  coef[8][8];      /* coef[o][c], Q30; entries outside [out)[in) are ignored */
} dvda_pcm_mix;               /* 264 bytes */
typedef struct dvda_pcm_mix_report {
    uint64_t frames;          /* PCM frames mixed */
    uint64_t clipped[8];      /* per OUTPUT channel: values the clamp changed */
} dvda_pcm_mix_report;        /* 72 bytes */

/* The tier-free form.  Stream i: d_desc_in[i] in d_in (layout_in) -> d_desc_out[i] in d_out (layout_out) through the
 * matrix d_mix[i], report d_report[i]; device arrays, n entries; each layout DVDA_PCM_PLANAR or DVDA_PCM_INTERLEAVED.
 * The matrices lie on the device, so the kernels judge them: a stream is taken only when its input descriptor is one
 * the reports take (channels 1..8, frames up to 2^40), its matrix is valid with in_channels == the input's channels and
 * out_channels == the output descriptor's channels, and the output descriptor says exactly the input's frames and a
 * stride >= frames; otherwise frames == 0 is reported and nothing is written.  Out of place only; any overlap of input
 * and output regions is the caller's error.  Enqueued on `stream`: no host wait, no allocation.  max_total_frames: a
 * bound the host knows on the sum of the streams' frames; a stream whose tiles (DVDA_LVL_TILE_FRAMES frames, aligned to
 * its start) fall outside it reports zeros, and its output region holds unspecified values inside its bounds and nothing
 * outside them.  d_work: dvda_pcm_hip_mix_workspace_words(n, max_total_frames) uint32 words, which need not be cleared;
 * no atomics, the report is the same from run to run.  Either side's off may have any 4-byte alignment and a planar
 * stride any parity; nothing outside a region's `frames` is read, nothing outside the output region written.  The
 * arguments are judged first, on any machine -- DVDA_HIP_EINVAL: bits outside {16, 20, 24}, a WAV layout on either
 * side, a null pointer, work_words too small; DVDA_HIP_ECAPACITY: 2^31 tiles or more -- then the device:
 * DVDA_HIP_ENODEV without one. */
size_t dvda_pcm_hip_mix_workspace_words(uint32_t n, uint64_t max_total_frames);
int dvda_pcm_hip_mix(const int32_t *d_in, uint32_t layout_in, const dvda_pcm_crc_desc *d_desc_in,
                     int32_t *d_out, uint32_t layout_out, const dvda_pcm_crc_desc *d_desc_out,
                     const dvda_pcm_mix *d_mix, uint32_t n, unsigned bits, uint64_t max_total_frames,
                     dvda_pcm_mix_report *d_report, uint32_t *d_work, size_t work_words, void *stream);

/* behind dvda_mlp_hip_decode (blocks): the first n streams of the last decode mixed into d_out, in the context's layout
 * on both sides (a WAV layout: DVDA_HIP_EINVAL): stream i through host_mix[i] (a host array of n matrices) to the dword
 * offset d_mix_off[i] with the planar stride d_mix_stride[i] (device arrays, as d_out_off / d_out_stride are; a stride
 * below the stream's frames: the stream is not taken).  Frames and channels are what dvda_mlp_hip_stream_info reports;
 * a matrix whose in_channels differs from that is a stream not taken.  A stream that carries DVDA_ST_OVERFLOW reports
 * zeros and nothing is written for it. */
int dvda_mlp_hip_pcm_mix(dvda_mlp_hip_ctx *ctx, const int32_t *d_pcm, const uint64_t *d_out_off, const uint64_t *d_out_stride,
                         int32_t *d_out, const uint64_t *d_mix_off, const uint64_t *d_mix_stride,
                         const dvda_pcm_mix *host_mix, unsigned bits, dvda_pcm_mix_report *host_report, uint32_t n,
                         void *stream);

/* Host helpers; none needs a device.
 * speaker_mask: the RIFF-WAVE speaker mask of DVD-Audio channel assignment 0..20 (what dvda_riff_wave_channel_mask of
 *   the disc tier answers: the table lives here), 0 for any other assignment.
 * mix_matrix: the default matrix above for a buffer whose channel c is the c-th set bit of speaker_mask, ascending, to
 *   out_channels = 1 or 2, flags = DVDA_MIX_NORMALIZED or DVDA_MIX_UNITY, | DVDA_MIX_LFE.  DVDA_HIP_EINVAL for a zero mask,
 *   bits outside 0x13F (FL FR FC LFE BL BR BC), out_channels outside {1, 2}, unknown flags or a NULL `out`.
 * mix_valid: 1 when the matrix is valid as stated above, else 0 (NULL: 0).
 * mix_value: the contract above for one output value -- the text the kernel compiles -- from the frame's in_channels
 *   values x; *clipped (may be NULL) = 1 when the clamp changed the value, else 0; an invalid matrix or depth, o >=
 *   out_channels or a NULL pointer: returns 0 and sets *clipped = -1. */
unsigned dvda_pcm_hip_speaker_mask(unsigned assignment);
int dvda_pcm_hip_mix_matrix(unsigned speaker_mask, uint32_t out_channels, uint32_t flags, dvda_pcm_mix *out);
int dvda_pcm_hip_mix_valid(const dvda_pcm_mix *m);
int32_t dvda_pcm_hip_mix_value(const int32_t *x, const dvda_pcm_mix *m, uint32_t o, unsigned bits, int *clipped);

/* ------------------------------------------------------------------ tier B */
/* The mlp.h mirror: same three calls, same meaning as reference src/mlp.h:29-42 /
 * src/mlp.c:265-354, with the reference's containers replaced by plain memory:
 *   stream_parameters  -> five unsigned codes (src/stream_parameters.h:23-29)
 *   BitstreamReader*   -> (data, len): the bytes the reference would enqueue (src/mlp.c:349-351)
 *   aa_int* samples    -> planar[c] points at the PCM frames decoded by THIS call for RIFF
 *                         channel c (valid until the next call); the binding appends them to
 *                         samples->_[c]
 * decode_packet returns the number of PCM frames decoded by the call; 0 = nothing decodable
 * yet (bytes stay queued) exactly as in the reference.  Where the reference assert()s, the
 * call returns 0 and dvda_hip_mlpdecoder_status() reports the DVDA_ST_* bits.
 * Compatibility tier: every call is a small GPU batch; use tier A for throughput. */
typedef struct dvda_hip_mlpdecoder dvda_hip_mlpdecoder;

dvda_hip_mlpdecoder *dvda_hip_open_mlpdecoder(unsigned group_0_bps, unsigned group_1_bps,
                                              unsigned group_0_rate, unsigned group_1_rate,
                                              unsigned channel_assignment, int device);
void dvda_hip_close_mlpdecoder(dvda_hip_mlpdecoder *decoder);
unsigned dvda_hip_mlpdecoder_decode_packet(dvda_hip_mlpdecoder *decoder, const uint8_t *data,
                                           size_t len, const int32_t **planar, unsigned *channels);
unsigned dvda_hip_mlpdecoder_status(const dvda_hip_mlpdecoder *decoder);
size_t dvda_hip_mlpdecoder_queued_bytes(const dvda_hip_mlpdecoder *decoder);
/* Which path the decoder is on.  0: its state lives on the device and a call decodes exactly the access units it was
 * given (one workgroup, csrc/mlp_coop.h k_coop<false, true>; csrc/mlp_step.h) -- the usual case.  1: the stream left what
 * that path takes (an access unit of non-standard length, src/mlp.c:719-738, or one larger than 4 KB) and every call
 * decodes from the stream's last major sync on through the batch tier, as rounds 1-3 did for every stream. */
int dvda_hip_mlpdecoder_path(const dvda_hip_mlpdecoder *decoder);

/* A group of n such decoders for a host that serves many streams at once (a ripper that reads several tracks in
 * parallel, a service with many listeners): the members share nothing -- each behaves, call for call, as if it had been
 * fed its packets alone through dvda_hip_mlpdecoder_decode_packet (returns, PCM, status, path, queued bytes; a member
 * never sees another's stream, state or failure) -- but one call on the group decodes every member's packet with ONE
 * launch pair, a workgroup per member, where n lone decoders pay n launch pairs one after the other.  (A call in which a
 * member brings more than 48 access units / 48 KB runs further launch pairs, "steps", again for all such members at
 * once; members on path 1 decode through the batch tier, one after the other.)  A HIP runtime failure of a step sets
 * DVDA_ST_DEVICE on every member that took part in it.
 * A group lives on ONE device and is used by ONE thread at a time.  It holds 229 KB of pinned host memory per member
 * from open to close (58.5 MB at DVDA_STREAM_GROUP_MAX). */
typedef struct dvda_hip_mlpdecoder_group dvda_hip_mlpdecoder_group;
#define DVDA_STREAM_GROUP_MAX 256u

/* n decoders (1 .. DVDA_STREAM_GROUP_MAX) on one device; NULL without a HIP device or with n out of range */
dvda_hip_mlpdecoder_group *dvda_hip_open_mlpdecoder_group(unsigned n, int device);
void dvda_hip_close_mlpdecoder_group(dvda_hip_mlpdecoder_group *group);
unsigned dvda_hip_mlpdecoder_group_size(const dvda_hip_mlpdecoder_group *group);
/* One call of dvda_hip_mlpdecoder_decode_packet for every member at once: member i is fed data[i][0, len[i])
 * (len[i] == 0 or data[i] == NULL: no packet for it this time).  frames[i] = what its own decode_packet would have
 * returned, planar[i * 6 + c] / channels[i] as there; the pointers are valid until the next call on the group.
 * frames, planar and channels may each be NULL.  Returns the sum of frames[]. */
unsigned long long dvda_hip_mlpdecoder_group_decode_packets(dvda_hip_mlpdecoder_group *group, const uint8_t *const data[],
                                                            const size_t len[], unsigned frames[],
                                                            const int32_t *planar[], unsigned channels[]);
/* member i's dvda_hip_mlpdecoder_status / _queued_bytes / _path (i >= n or group == NULL: all-ones / 0 / -1) */
unsigned dvda_hip_mlpdecoder_group_status(const dvda_hip_mlpdecoder_group *group, unsigned i);
size_t dvda_hip_mlpdecoder_group_queued_bytes(const dvda_hip_mlpdecoder_group *group, unsigned i);
int dvda_hip_mlpdecoder_group_path(const dvda_hip_mlpdecoder_group *group, unsigned i);
/* how many steps (launch pairs) the group has run so far: what a caller pays */
unsigned long long dvda_hip_mlpdecoder_group_steps(const dvda_hip_mlpdecoder_group *group);

#ifdef __cplusplus
}
#endif
#endif
