/* dvd-audio-hip.h -- tier C of the HIP decoder: the disc-level API (SURVEY.md 8(b) "outer
 * boundary", rows f-1 and f-4), exported by libdvd_audio_hip.so.
 *
 * The 27 entry points below have the names, argument meaning, 1-based numbering, NULL-on-failure
 * and ownership rules of the reference's public header (reference include/dvd-audio.h:59-201),
 * so a program written against that header -- utils/dvda2wav.c for one -- links against this
 * library unchanged.  What differs is the inside: a track's AOB sectors are read, uploaded and decoded
 * on the GPU in batches
 *
 *     sector walk + payload gather   (reference src/packet.c:61-188, src/dvd-audio.c:1151-1248)
 *     major-sync search, end-of-track rule            (src/dvd-audio.c:1167-1194, 1238-1421)
 *     MLP decode (tier A of dvda_mlp_hip.h)  /  PCM un-swizzle      (src/mlp.c, src/pcm.c:99-193)
 *
 * -- a track of at most DVDA_WINDOW_SECTORS sectors (default 8 192 = 16 MiB) as ONE batch when its reader is
 * opened; a longer one, MLP or raw PCM, window by window: a producer thread reads, demultiplexes and decodes
 * window k + 1 into one of two pinned buffers while dvda_read() / dvda_hip_reader_wav_next() hand out window k,
 * so what a reader holds is bounded by the window, not by the track (the reference streams a track packet by
 * packet, src/dvd-audio.c:752-795).  There is no CPU decode path: a
 * track reader cannot be opened without a HIP device.  CPPM-protected discs are not handled
 * (`device` is accepted and ignored; reference src/aob.c:109-127).
 */
#ifndef DVD_AUDIO_HIP_H
#define DVD_AUDIO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DVDA_HIP_PTS_PER_SECOND 90000

typedef struct DVDA_s DVDA;
typedef struct DVDA_Titleset_s DVDA_Titleset;
typedef struct DVDA_Title_s DVDA_Title;
typedef struct DVDA_Track_s DVDA_Track;
typedef struct DVDA_Track_Reader_s DVDA_Track_Reader;

typedef enum { DVDA_PCM, DVDA_MLP } dvda_codec_t;

/* ---- disc: AUDIO_TS.IFO (reference src/dvd-audio.c:323-360, 896-930) */
DVDA *dvda_open(const char *audio_ts_path, const char *device);
void dvda_close(DVDA *dvda);
unsigned dvda_titleset_count(const DVDA *dvda);

/* ---- titleset: ATS_XX_0.IFO (src/dvd-audio.c:362-424, 932-1014) */
DVDA_Titleset *dvda_open_titleset(DVDA *dvda, unsigned titleset);
void dvda_close_titleset(DVDA_Titleset *titleset);
unsigned dvda_titleset_number(const DVDA_Titleset *titleset);
unsigned dvda_title_count(const DVDA_Titleset *titleset);

/* ---- title: track table and the sector range of every track (src/dvd-audio.c:426-515) */
DVDA_Title *dvda_open_title(DVDA_Titleset *titleset, unsigned title);
void dvda_close_title(DVDA_Title *title);
unsigned dvda_title_number(const DVDA_Title *title);
unsigned dvda_track_count(const DVDA_Title *title);
unsigned dvda_title_pts_length(const DVDA_Title *title);

/* ---- track (src/dvd-audio.c:517-584) */
DVDA_Track *dvda_open_track(DVDA_Title *title, unsigned track);
void dvda_close_track(DVDA_Track *track);
unsigned dvda_track_number(const DVDA_Track *track);
unsigned dvda_track_pts_index(const DVDA_Track *track);
unsigned dvda_track_pts_length(const DVDA_Track *track);
unsigned dvda_track_first_sector(const DVDA_Track *track);
unsigned dvda_track_last_sector(const DVDA_Track *track);

/* ---- track reader (src/dvd-audio.c:586-794): a short track is decoded when its reader is opened, a long one in
 *      windows while it is read (see the top of this file; dvda_hip_reader_windowed()) */
DVDA_Track_Reader *dvda_open_track_reader(const DVDA_Track *track);
void dvda_close_track_reader(DVDA_Track_Reader *reader);
dvda_codec_t dvda_codec(const DVDA_Track_Reader *reader);
unsigned dvda_bits_per_sample(const DVDA_Track_Reader *reader);
unsigned dvda_sample_rate(const DVDA_Track_Reader *reader);
unsigned dvda_channel_count(const DVDA_Track_Reader *reader);
unsigned dvda_riff_wave_channel_mask(const DVDA_Track_Reader *reader);
/* interleaved int samples in RIFF-WAVE channel order; returns the PCM frames delivered, fewer
 * than asked only at the end of the track, 0 afterwards */
unsigned dvda_read(DVDA_Track_Reader *reader, unsigned pcm_frames, int buffer[]);

/* ---- additions of this library (not in the reference API) */
/* HIP device used by track readers opened afterwards (default 0) */
void dvda_hip_set_device(int device);
/* on != 0: MLP track readers opened afterwards are decoded straight into the WAV payload dvda2wav would write
 * (the output stage -- dvda_read's interleave + write_signed at the stream's bit depth -- runs inside the decode
 * kernels, DVDA_PCM_WAV24 / DVDA_PCM_WAV16): no int32 PCM buffer, no packing pass.  Such a reader serves
 * dvda_hip_reader_wav_payload() only; dvda_read() on it returns 0 (dvda_hip_reader_wav_only() tells that case from an
 * empty track).  Default off (the reference API's int samples). */
void dvda_hip_set_wav_output(int on);
/* Both options are per calling THREAD (a host that fans tracks out over several devices sets them in each worker).
 * The per-reader form: opens the track on HIP device `device`, as a WAV-payload-only reader if wav_output != 0,
 * whatever the thread's defaults are, and leaves those alone. */
DVDA_Track_Reader *dvda_hip_open_track_reader_on(const DVDA_Track *track, int device, int wav_output);
/* presentation = 1: MLP track readers opened afterwards (per calling thread, like dvda_hip_set_wav_output) decode the
 * 2-channel presentation of a two-substream title -- substream 0 alone, DVDA_PRESENT_SUBSTREAM0 of dvda_mlp_hip.h, where
 * the rule is stated: what a 2-channel player plays from a multichannel disc, not channels 0 and 1 of the full decode.
 * dvda_channel_count() then returns k (substream 0's channels; 2 on such discs), dvda_riff_wave_channel_mask() the mask of
 * the identity assignment of k channels (0x3 for k = 2), and dvda_read() / dvda_hip_reader_wav_payload() /
 * dvda_hip_reader_wav_next() deliver k-channel frames.  One-substream MLP tracks and raw-PCM tracks are read as always.
 * 0 (default): the full decode. */
void dvda_hip_set_presentation(int presentation);
/* dvda_hip_open_track_reader_on with the presentation named too; the thread's defaults stay as they are (conceal mode
 * is the thread's, or DVDA_CONCEAL's while the thread has not chosen: dvda_hip_set_conceal below) */
DVDA_Track_Reader *dvda_hip_open_track_reader_with(const DVDA_Track *track, int device, int wav_output, int presentation);
/* on != 0: track readers opened afterwards (per calling thread, read when the reader is opened, like
 * dvda_hip_set_wav_output) digest every piece of the track where it lies on the device, before any copy to the host:
 * zlib's CRC-32 of the WAV data chunk dvda2wav writes for the track (the contract is in dvda_mlp_hip.h,
 * dvda_pcm_hip_crc32).  Whole-track and windowed readers, MLP and raw-PCM tracks, int32 and WAV-payload output, the
 * presentation.  Off (default): a reader launches and allocates exactly as without this call. */
void dvda_hip_set_digest(int on);
/* The track's digest and its payload bytes.  1: final for the track -- from open on for a whole-track reader, once the
 * track has been read to its end for a windowed one (which joins its windows' digests as they are handed out: until
 * then 0, with the digest of what has been handed out so far).  -1: the digest is not on, the reader failed, or the
 * track's bit depth is neither 16 nor 24. */
int dvda_hip_reader_crc32(const DVDA_Track_Reader *reader, unsigned *crc, unsigned long long *bytes);
/* on != 0: track readers opened afterwards (per calling thread, read when the reader is opened, exactly like
 * dvda_hip_set_digest) make the level report of every piece of int32 PCM where it lies on the device, before any copy
 * to the host: per channel min, max, exact sum and the values outside the nominal range of the track's
 * dvda_bits_per_sample, and the frames of digital silence at both ends (the contract is in dvda_mlp_hip.h,
 * dvda_pcm_levels / dvda_pcm_hip_levels).  Every reader that holds int32 PCM: whole-track and windowed, MLP and raw PCM,
 * the presentation.  A reader opened for the WAV payload only holds no int32 PCM and has no report (dvda2wav_hip's
 * readers are such readers: the extractor is out of scope).  Off (default): a reader launches and allocates exactly
 * as without this call. */
struct dvda_pcm_levels;
void dvda_hip_set_levels(int on);
/* The track's report.  1: final for the track -- from open on for a whole-track reader, once the track has been read
 * to its end for a windowed one (which joins its windows' reports as they are handed out, dvda_pcm_hip_levels_combine:
 * until then 0, with the report of what has been handed out so far).  -1: the report is not on, the reader failed, it
 * is a WAV-payload-only reader (dvda_hip_reader_wav_only), or the track's bit depth is none of 16 / 20 / 24.  `out` may
 * be NULL. */
int dvda_hip_reader_levels(const DVDA_Track_Reader *reader, struct dvda_pcm_levels *out);
/* block_frames != 0: track readers opened afterwards (per calling thread, read when the reader is opened, like
 * dvda_hip_set_levels) make the energy report of every piece of int32 PCM where it lies on the device, before any copy
 * to the host: per block of block_frames frames and channel the exact sum of squares and the largest |v| (the contract
 * is in dvda_mlp_hip.h, dvda_pcm_energy_block / dvda_pcm_hip_energy).  The grid is the track's, anchored at track frame
 * 0: a windowed reader gives every window the lead that is left of the block the track is in, and joins the windows'
 * blocks as they are handed out (dvda_pcm_hip_energy_append); conceal mode's silent windows are pieces like any other.
 * Every reader that holds int32 PCM: whole-track and windowed, MLP and raw PCM, the presentation.  A reader opened for
 * the WAV payload only has no report, nor has one opened with a block_frames outside DVDA_NRG_MIN_BLOCK ..
 * DVDA_NRG_MAX_BLOCK.  0 (default): off, a reader launches and allocates exactly as without this call. */
struct dvda_pcm_energy_block;
void dvda_hip_set_energy(unsigned block_frames);
/* The track's blocks: up to `cap` of them into `blocks` (may be NULL), their count into *n (may be NULL).  1: final for
 * the track; 0: the blocks of what has been handed out so far (a windowed reader; the last of them may still grow);
 * -1: the report is not on, the reader failed, or it is a WAV-payload-only reader -- nothing is written.  The track's
 * block array is the report itself (168 bytes per block, on the host): it is not part of the window-bounded host
 * figure of dvda_hip_reader_memory. */
int dvda_hip_reader_energy(const DVDA_Track_Reader *reader, struct dvda_pcm_energy_block *blocks, unsigned long long cap,
                           unsigned long long *n);
/* bits_out != 0 (16, 20 or 24): track readers opened afterwards (per calling thread, read when the reader is opened,
 * like dvda_hip_set_levels) deliver the track at that word length: every piece of int32 PCM is reduced where it lies on
 * the device -- mode: DVDA_RQ_TRUNCATE, DVDA_RQ_ROUND or DVDA_RQ_TPDF with `seed`, and clamped to the output range; the
 * contract is in dvda_mlp_hip.h, dvda_pcm_requant / dvda_pcm_hip_requantize -- with frame0 = the track's frames in front
 * of the piece, so a track read whole and one read in windows are the same bytes.  Everything behind it describes what
 * the reader hands out: the digest, the level and energy reports, the WAV payload, dvda_read; dvda_bits_per_sample()
 * returns bits_out.  A reader that would decode straight into the WAV payload (dvda_hip_set_wav_output) decodes int32
 * instead and is packed at bits_out afterwards.  Every reader: whole-track and windowed, MLP and raw PCM, the
 * presentation.  A track whose depth is below bits_out is handed out as it is (the option is off for that reader); one
 * whose depth equals bits_out is clamped and nothing else.  Out of scope: together with conceal mode (the stitch between
 * two windows rewrites frames already handed over) -- such an open returns NULL, as does one with a bits_out or mode
 * the reduction does not have.  0 (default): off, a reader launches and allocates exactly as without this call. */
struct dvda_pcm_requant_report;
void dvda_hip_set_requantize(unsigned bits_out, unsigned mode, unsigned long long seed);
/* What the reduction counted: frames and, per channel, the values the clamp changed.  1: final for the track; 0: of what
 * has been handed out so far (a windowed reader); -1: the reader does not reduce -- opened without the option, or the
 * track's depth is below bits_out -- or it failed; nothing is written.  `out` may be NULL. */
int dvda_hip_reader_requantized(const DVDA_Track_Reader *reader, struct dvda_pcm_requant_report *out);
/* the depth the track has on the disc: dvda_bits_per_sample() unless the reader reduces the word length */
unsigned dvda_hip_reader_source_bits(const DVDA_Track_Reader *reader);
/* ratio 2 or 4: track readers opened afterwards (per calling thread, read when the reader is opened, like
 * dvda_hip_set_requantize) deliver a track at its rate / ratio where that is 44 100, 48 000, 88 200 or 96 000 Hz: the
 * decoded int32 PCM is decimated on the device into a second buffer at the track's depth -- the contract, an exact
 * integer FIR with one rounding and a clamp, is in dvda_mlp_hip.h, dvda_pcm_hip_decimate -- and from there on the reader
 * IS a track of ceil(F / ratio) frames at the lower rate: the word-length reduction (its frame0 counts output frames),
 * the digest, the level and energy reports, the WAV payload, dvda_read, dvda_hip_reader_total_frames() and
 * dvda_sample_rate() all describe the decimated track.  A reader that would decode straight into the WAV payload
 * decodes int32 instead and is packed afterwards.  Any other track (48 kHz by 2, 96 kHz by 4) is handed out as it is.
 * Whole-track readers only, MLP and raw PCM: a track the reader would take in windows makes the open return NULL, and so
 * does the option together with conceal mode or a ratio other than 0, 2 and 4.  (dvda_pcm_decim_piece already carries
 * what decimating window by window needs.)  0 (default): off, a reader launches and allocates exactly as without. */
struct dvda_pcm_decim_report;
void dvda_hip_set_decimate(unsigned ratio);
/* 1: the reader decimates (also: as the first stage of dvda_hip_set_resample), *out (may be NULL) = what the pass
 * counted (frames in and out, per channel the values the clamp changed); 0: it does not -- the option is off, the
 * track's rate is not one it applies to, or `reader` is NULL; nothing is written */
int dvda_hip_reader_decimated(const DVDA_Track_Reader *reader, struct dvda_pcm_decim_report *out);
/* the rate the track has on the disc: dvda_sample_rate() unless the reader decimates or resamples; 0 for a NULL reader */
unsigned dvda_hip_reader_source_rate(const DVDA_Track_Reader *reader);
/* rate 44100: track readers opened afterwards (per calling thread, read when the reader is opened, like
 * dvda_hip_set_decimate) deliver a 48 / 96 / 192 kHz track at 44 100 Hz: the decoded int32 PCM is decimated by rate /
 * 48 000 where that is above 1 (dvda_pcm_hip_decimate, at the track's depth), then resampled by 147 / 160 into a new
 * buffer (dvda_pcm_hip_resample: the contract, an exact integer polyphase FIR with one rounding and a clamp at the track's
 * depth, is in dvda_mlp_hip.h), and from there on the reader IS the 44.1 kHz track of ceil(147 F / 160) frames for the
 * word-length reduction, the reports, the WAV payload, dvda_read, dvda_hip_reader_total_frames() and dvda_sample_rate()
 * (44 100); dvda_hip_reader_source_rate() gives the disc's rate.  Any other track (the 44.1 kHz family) is handed out as
 * it is.  Whole-track readers only, MLP and raw PCM: the open returns NULL for a track the reader would take in windows,
 * in conceal mode, together with a non-zero dvda_hip_set_decimate, and for any value but 0 and 44100.  0 (default): off. */
void dvda_hip_set_resample(unsigned rate);
/* 1: the reader resamples, *out (may be NULL) = what the 48 -> 44.1 kHz pass counted (frames in at 48 kHz and out, per
 * channel the values the clamp changed) -- where the track ran at 96 / 192 kHz, dvda_hip_reader_decimated gives the stage
 * in front of it; 0: it does not -- the option is off, the track's rate is not one it applies to, or `reader` is NULL;
 * nothing is written */
int dvda_hip_reader_resampled(const DVDA_Track_Reader *reader, struct dvda_pcm_decim_report *out);
/* out_channels 1 or 2: track readers opened afterwards (per calling thread, read when the reader is opened, like
 * dvda_hip_set_decimate) deliver a track of any other channel count mixed to that many channels: the decoded int32 PCM
 * goes through dvda_pcm_hip_mix with the default matrix of the track's channel assignment (dvda_pcm_hip_mix_matrix of
 * dvda_pcm_hip_speaker_mask(assignment) with `flags`, DVDA_MIX_*: the contract is in dvda_mlp_hip.h) at the track's depth
 * into a new buffer, FIRST -- in front of the decimation, the resampler, the word-length reduction and the reports, which
 * all see the mixed track; every stage rounds and clamps, so this order is part of the contract.  From there on the
 * reader IS the 1- or 2-channel track: dvda_channel_count() gives out_channels, dvda_riff_wave_channel_mask() FL | FR
 * (mono: FC), dvda_hip_reader_source_channels() the disc's count.  A track that already has out_channels channels -- a
 * stereo presentation through dvda_hip_set_presentation(1) too -- is handed out untouched.  Whole-track readers only, MLP
 * and raw PCM: the open returns NULL for a track the reader would take in windows, in conceal mode, for out_channels above
 * 2, unknown flags, and for flags whose matrix the kernels do not take (dvda_pcm_hip_mix_valid: DVDA_MIX_UNITY on 5.0 /
 * 5.1).  0 (default): off. */
struct dvda_pcm_mix_report;
void dvda_hip_set_downmix(unsigned out_channels, unsigned flags);
/* 1: the reader mixes, *out (may be NULL) = what the pass counted (frames, per OUTPUT channel the values the clamp
 * changed); 0: it does not -- the option is off, the track has out_channels channels already, or `reader` is NULL; nothing
 * is written */
int dvda_hip_reader_downmixed(const DVDA_Track_Reader *reader, struct dvda_pcm_mix_report *out);
/* the channels the track has on the disc: dvda_channel_count() unless the reader mixes; 0 for a NULL reader */
unsigned dvda_hip_reader_source_channels(const DVDA_Track_Reader *reader);
/* on != 0: MLP track readers opened afterwards (per calling thread, read when the reader is opened, like
 * dvda_hip_set_wav_output) conceal a damaged track instead of refusing it: the track comes out as
 *     kept PCM ++ silence ++ PCM of a fresh decoder from the next usable major sync ++ ...
 * exactly as conceal mode of the batch tier composes the track's whole MLP stream (the rule is in dvda_mlp_hip.h,
 * dvda_mlp_hip_set_conceal).  The stream is the bytes the demux yields for the track's sectors, from the first
 * major-sync pattern to the end-of-track rule; a sector the demux refuses (zero-filled, a bad pack header) contributes
 * no bytes, and the codec probe skips a malformed sector inside the track.  dvda_read(), both payload calls, the digest
 * and the level report see the composed track -- the silence is exact zeros.  A clean track reads exactly as without the
 * option.  While this call has not been made on the thread, DVDA_CONCEAL=1 in the environment turns the option on: a
 * program written against the reference's header -- its dvda2wav, linked against this library -- extracts a damaged
 * disc that way.
 * A long track is read in windows of bounded memory as without the option: each window is concealed on its own and the
 * reader stitches what lies between two windows (history, silence, spans), so the track comes out as it would from one
 * batch.  One stated exception: a hole of 65 536 frames or more takes its 65 536-frame wrap count from the mean bytes per
 * frame of the track so far, not of the whole stream.
 * Scope: together with the 2-channel presentation (dvda_hip_set_presentation(1)) the batch tier
 * refuses conceal mode, and an MLP track reader does not open.  Raw-PCM tracks are read as always: a lost sector still
 * shortens them.  Off (default): a reader launches, allocates and fails exactly as without this call.
 * Lost sectors and alignment: a sector carries 2 021 MLP bytes and access units start at even offsets of the stream, so an
 * odd number of sectors lost in a row leaves every unit behind them at an odd offset, where the index does not look: the
 * rest of the track is then one TRAILING span.  An even number (and any damage inside sectors) resumes at the next usable
 * major sync. */
struct dvda_mlp_conceal_span;
void dvda_hip_set_conceal(int on);
/* dvda_hip_open_track_reader_with with conceal mode named too: 1 on, 0 off, < 0 as the thread (or DVDA_CONCEAL) has it;
 * the thread's defaults stay as they are */
DVDA_Track_Reader *dvda_hip_open_track_reader_concealing(const DVDA_Track *track, int device, int wav_output, int presentation,
                                                         int conceal);
/* What was concealed of the track: up to cap spans (dvda_mlp_conceal_span of dvda_mlp_hip.h) into spans, *n = how many
 * there are (none for a clean track); in track terms -- PCM frames of the track, byte offsets from the first byte of the
 * track's stream.  1: final for the track (from open on for a whole-track reader), 0: not yet final (a windowed
 * reader before its last window has been produced: the spans so far), -1: the reader was opened without conceal mode.  dvda_hip_reader_status() carries
 * DVDA_ST_CONCEALED once a span exists.  spans may be NULL with cap 0 (the count call). */
int dvda_hip_reader_concealed(const DVDA_Track_Reader *reader, struct dvda_mlp_conceal_span *spans, unsigned cap, unsigned *n);
/* != 0: the reader holds the WAV payload only (opened with wav_output): dvda_read() on it returns 0 frames -- NOT
 * because the track is empty; take the payload with dvda_hip_reader_wav_payload() */
int dvda_hip_reader_wav_only(const DVDA_Track_Reader *reader);
/* ---- long tracks (round 5).  An MLP track of more than a window of sectors (DVDA_WINDOW_SECTORS in the environment,
 * default 8192 = 16 MiB) is read, demultiplexed and decoded window by window while it is served, as the reference
 * streams it (src/dvd-audio.c:751-795): what is resident on the host and on the device is bounded by the window, not
 * by the track.  dvda_read() works on such a reader as on any other.  Its WAV payload comes piece by piece: */
/* the next piece of the track's WAV data bytes (valid until the next call on this reader); 0 at the end of the track.
 * (A reader that is not windowed hands out its whole payload in one piece, once.) */
unsigned long long dvda_hip_reader_wav_next(DVDA_Track_Reader *reader, const unsigned char **payload);
/* != 0: the reader decodes in windows (dvda_hip_reader_total_frames() is then the count so far: final when the
 * track has been read to its end) */
int dvda_hip_reader_windowed(const DVDA_Track_Reader *reader);
/* != 0: a window of the track could not be read or decoded (what makes dvda_open_track_reader return NULL when it
 * happens in a track's first window): dvda_read() / dvda_hip_reader_wav_next() then end early */
int dvda_hip_reader_failed(const DVDA_Track_Reader *reader);
/* peaks of what a windowed reader held: bytes of host memory it allocated (pinned buffers, the bytes kept between
 * windows), and of device memory in use beyond what was in use when it was opened (hipMemGetInfo, sampled after every
 * window); returns 0 on a reader that is not windowed */
int dvda_hip_reader_memory(const DVDA_Track_Reader *reader, unsigned long long *host_peak, unsigned long long *device_peak);
/* A windowed reader's decode context, device buffers and pinned buffers are kept, when it is closed, by the closing thread
 * for the next windowed reader that thread opens on the same device (one set per thread).  This frees the calling
 * thread's set; a thread that opens no more readers calls it before it ends. */
void dvda_hip_release_cached_buffers(void);
/* status word of the decode behind a reader: DVDA_ST_* bits of dvda_mlp_hip.h (0 = clean) */
unsigned dvda_hip_reader_status(const DVDA_Track_Reader *reader);
/* PCM frames the reader holds in total */
unsigned long long dvda_hip_reader_total_frames(const DVDA_Track_Reader *reader);
/* The rest of the track as the WAV payload dvda2wav would write for it (interleaved,
 * little-endian, write_signed semantics, packed on the GPU): returns the byte count and a
 * pointer valid until the reader is closed; the reader is at its end afterwards. */
unsigned long long dvda_hip_reader_wav_payload(DVDA_Track_Reader *reader, const unsigned char **payload);

#ifdef __cplusplus
}
#endif
#endif
