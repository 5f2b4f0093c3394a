/* disc_reader.c -- the disc tier's track readers (include/dvd-audio-hip.h), host side, plain C.  Built into
 * libdvd_audio_hip.so with disc_ifo.c (the IFO walk and the AOB files) on top of libdvda_mlp_hip.so.
 *
 * Mirrors what reference src/dvd-audio.c + src/packet.c do (SURVEY.md 8(b) outer boundary, rows f-1 and f-4), with the
 * per-packet decode loop replaced by one GPU batch per track, or per window of a long track:
 *
 *   codec probe         first 0xBD packet at/after the track's first sector (src/dvd-audio.c:586-655)
 *   MLP track           sectors -> GPU gather of the MLP payload (sectors_to_device); stream start = first major
 *                       sync found byte by byte (locate_mlp_parameters, src/dvd-audio.c:1327-1365); stream end = the
 *                       first major sync at or after the first payload byte of a sector beyond the track's last
 *                       sector (stream_bounds; decode_mlp_audio + mlp_data_to_major_sync, src/dvd-audio.c:1167-1194,
 *                       1367-1421); then tier A index + decode of that one stream (index_stream, decode_stream)
 *   PCM track           sectors -> GPU un-swizzle (sectors_to_device); whole packets are delivered until
 *                       lround(PTS length * rate / 90000) frames are covered (pcm_deliver; open_pcm_track_reader /
 *                       decode_pcm_audio, src/dvd-audio.c:958-1084)
 *   dvda_read           interleave out of the decoded track (src/dvd-audio.c:757-794)
 *
 * Each of these steps is written once and takes a buffer set (struct track_bufs); the two kinds of reader -- a track
 * as one batch (open_mlp, open_pcm), a long track window by window (win_produce, win_produce_pcm) -- are sequences of
 * them and differ in who owns the buffers and how long.
 *
 * Streams the reference would abort on (assert) make dvda_open_track_reader return NULL here -- unless the reader is
 * opened in conceal mode (dvda_hip_set_conceal): the decode then composes kept PCM and silence (conceal mode of the batch
 * tier), and the windowed reader stitches what lies between two windows (win_conceal_stitch).
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/dvda_mlp_hip.h"
#include "disc_internal.h"

#define CODEC_PCM 0xA0u
#define CODEC_MLP 0xA1u

/* What a reader is opened with.  The defaults are per THREAD: a host that fans tracks out over several devices
 * (tools/dvda2wav_hip.c --devices) sets them in each of its worker threads.  dvda_open_track_reader() copies them once
 * and hands the copy down; dvda_hip_open_track_reader_on() / _with() name their own and touch none of the defaults. */
struct reader_opts {
    int device;
    int wav_output;             /* 1: MLP readers decode straight into the WAV payload */
    int present;                /* 1: MLP readers decode the presentation substream 0 carries (DVDA_PRESENT_SUBSTREAM0) */
    int digest;                 /* 1: every piece of PCM is digested where it lies on the device (dvda_hip_reader_crc32) */
    int levels;                 /* 1: ... and its level report is made there (dvda_hip_reader_levels) */
    int conceal;                /* 1: a damaged MLP track is concealed, not refused (dvda_hip_set_conceal) */
    unsigned energy;            /* != 0: ... and its energy report on a grid of that many frames (dvda_hip_reader_energy) */
    unsigned rq_bits, rq_mode;  /* rq_bits != 0: every piece of int32 PCM is reduced to that many bits where it lies on the */
    unsigned long long rq_seed; /*   device, in front of its reports (dvda_hip_set_requantize, dvda_hip_reader_requantized) */
    unsigned dc_ratio;          /* != 0: a whole-track reader decimates the decoded PCM by 2 or 4 on the device, in front of
                                   all of the above (dvda_hip_set_decimate, dvda_hip_reader_decimated) */
    unsigned rs_rate;           /* != 0 (44100): a whole-track reader brings a 48 / 96 / 192 kHz track to 44.1 kHz on the device,
                                   in the decimation's place (dvda_hip_set_resample, dvda_hip_reader_resampled) */
    unsigned mx_ch, mx_flags;   /* mx_ch != 0 (1, 2): a whole-track reader mixes a track of another channel count to that many
                                   channels on the device, in front of all of the above (dvda_hip_set_downmix,
                                   dvda_hip_reader_downmixed) */
};
static _Thread_local struct reader_opts t_opts;
static _Thread_local int t_conceal_set;     /* dvda_hip_set_conceal() was called on this thread: DVDA_CONCEAL no longer counts */
void dvda_hip_set_device(int device) { t_opts.device = device; }
void dvda_hip_set_wav_output(int on) { t_opts.wav_output = on != 0; }
void dvda_hip_set_presentation(int presentation) { t_opts.present = presentation == 1; }
void dvda_hip_set_digest(int on) { t_opts.digest = on != 0; }
void dvda_hip_set_levels(int on) { t_opts.levels = on != 0; }
void dvda_hip_set_energy(unsigned block_frames) { t_opts.energy = block_frames; }
void dvda_hip_set_requantize(unsigned bits_out, unsigned mode, unsigned long long seed)
{
    t_opts.rq_bits = bits_out;
    t_opts.rq_mode = mode;
    t_opts.rq_seed = seed;
}
void dvda_hip_set_decimate(unsigned ratio) { t_opts.dc_ratio = ratio; }
void dvda_hip_set_resample(unsigned rate) { t_opts.rs_rate = rate; }
void dvda_hip_set_downmix(unsigned out_channels, unsigned flags)
{
    t_opts.mx_ch = out_channels;
    t_opts.mx_flags = flags;
}
void dvda_hip_set_conceal(int on)
{
    t_opts.conceal = on != 0;
    t_conceal_set = 1;
}

/* the calling thread's options as a reader opened now gets them: while the thread has not said what it wants of conceal
 * mode, DVDA_CONCEAL=1 in the environment turns it on (a program written against the reference's header has no call
 * for it) */
static struct reader_opts opts_now(void)
{
    struct reader_opts o = t_opts;
    if (!t_conceal_set) {
        const char *e = getenv("DVDA_CONCEAL");
        o.conceal = e && e[0] == '1' && e[1] == 0;
    }
    return o;
}

struct track_windows;               /* a long track read window by window (below) */

/* The reports of a piece of PCM or of a track: the digest (dvda_hip_set_digest), the level report
 * (dvda_hip_set_levels), the energy report (dvda_hip_set_energy) and what the word-length reduction counted
 * (dvda_hip_set_requantize).  Per report a state -- 0 off, 1 wanted and, once a
 * piece is through, made (a windowed track: joined over the windows handed out so far), -1 this reader has none -- and
 * its values.  The energy report's blocks are the record's own (rep_reset frees them): a piece's lie on the track's
 * grid, which is anchored at track frame 0, and join the track's when the piece is handed out. */
struct pcm_reports {
    int dg, lv, ng;
    uint32_t crc;               /* zlib CRC-32 of the WAV payload and its bytes */
    uint64_t bytes;
    dvda_pcm_levels levels;
    uint32_t ng_block;          /* the grid's block length */
    dvda_pcm_energy_block *ng_blocks;
    uint64_t ng_n, ng_cap;
    int rq;                     /* the word-length reduction: 0 also for a track whose depth is below bits_out */
    dvda_pcm_requant rq_par;    /* (bits_in: set per piece from the track's depth) */
    dvda_pcm_requant_report rq_rep;
};

/* the reports a reader opened with `o` wants */
static void rep_want(struct pcm_reports *r, const struct reader_opts *o)
{
    r->dg = o->digest;
    r->lv = o->levels;
    r->ng = o->energy != 0;
    r->ng_block = o->energy;
    r->rq = o->rq_bits != 0;
    r->rq_par.bits_in = r->rq_par.bits_out = o->rq_bits;
    r->rq_par.mode = o->rq_mode;
    r->rq_par.reserved = 0;
    r->rq_par.seed = o->rq_seed;
}

/* does a reader opened with `o` reduce a track of `bits` bits?  (a track below bits_out is handed out as it is) */
static int rq_applies(const struct reader_opts *o, unsigned bits) { return o->rq_bits != 0 && bits >= o->rq_bits; }
static unsigned code_of_bits(unsigned bits) { return bits == 16 ? 0 : bits == 20 ? 1 : 2; }

/* does a reader opened with `o` decimate a track whose rate has `rate_code`?  Only where rate / ratio is one of 44 100,
 * 48 000, 88 200, 96 000: the codes count 0, 1, 2 = x1, x2, x4 inside a rate family (bit 3), so the quotient's code is
 * rate_code - log2(ratio) where that is not negative.  Any other track is handed out as it is. */
static unsigned dc_shift(const struct reader_opts *o) { return o->dc_ratio == 2 ? 1 : o->dc_ratio == 4 ? 2 : 0; }
static int dc_applies(const struct reader_opts *o, unsigned rate_code)
{
    return dc_shift(o) != 0 && rate_of(rate_code) != 0 && (rate_code & 3) >= dc_shift(o);
}

/* does a reader opened with `o` resample a track whose rate has `rate_code`?  The 48 kHz family (bit 3 clear): 48 kHz as
 * it is, 96 / 192 kHz decimated by 2 / 4 first.  Any other track is handed out as it is. */
static int rs_applies(const struct reader_opts *o, unsigned rate_code)
{
    return o->rs_rate == 44100 && rate_of(rate_code) != 0 && !(rate_code & 8);
}

/* does a reader opened with `o` mix a track of `channels` channels?  (a track that has out_channels already -- a stereo
 * presentation too -- is handed out as it is) */
static int mx_applies(const struct reader_opts *o, unsigned channels) { return o->mx_ch != 0 && channels != o->mx_ch; }

static void rep_reset(struct pcm_reports *r)
{
    free(r->ng_blocks);
    memset(r, 0, sizeof(*r));
}

struct DVDA_Track_Reader_s {
    dvda_codec_t codec;
    struct track_windows *win;     /* != NULL: the track is decoded in windows of bounded size as it is read */
    unsigned bps_code[2], rate_code[2], assignment;
    unsigned channels, status;
    unsigned src_bits;         /* != 0: the track's own depth, where the reader hands out fewer bits (dvda_hip_set_requantize) */
    unsigned src_rate;         /* != 0: the track's own rate, where the reader hands out a lower one (dvda_hip_set_decimate,
                                  dvda_hip_set_resample) */
    int dc_done, rs_done;      /* the track went through the decimation / the resampler */
    unsigned src_channels;     /* != 0: the track's own channel count, where the reader hands out the mix (dvda_hip_set_downmix) */
    dvda_pcm_mix_report mx_rep;    /* ... and what the mix counted */
    dvda_pcm_decim_report dc_rep, rs_rep;      /* ... and what each counted */
    uint64_t frames, served, stride;
    int interleaved;           /* MLP tracks: frame-major [frame][channel] = the dvda_read order;
                                  PCM tracks: planar [channel][stride]; RIFF-WAVE channel order */
    int32_t *pcm;              /* host copy of d_pcm, made by the first dvda_read() */
    int32_t *d_pcm;            /* device copy, kept for the GPU WAV packer */
    uint8_t *wav;              /* host payload produced by dvda_hip_reader_wav_payload */
    uint8_t *d_wav;            /* MLP reader opened for the payload: the decode kernels wrote the WAV payload
                                  themselves (DVDA_PCM_WAV24 / WAV16); there is no int32 PCM for dvda_read() */
    uint64_t wav_bytes;
    struct pcm_reports rep;    /* a whole-track reader: the track's */
    int conceal;               /* opened in conceal mode (dvda_hip_set_conceal) */
    dvda_mlp_conceal_span *spans;      /* ... and what was concealed, in track terms (dvda_hip_reader_concealed) */
    unsigned n_spans;
};

/* fills the reader's record from the index's stream record; 0 = a channel count the assignment does not have.  Under
 * the presentation a two-substream stream has k channels in the identity assignment of k (MLP channel c = RIFF channel
 * c, src/mlp.c:416-438), whatever its major sync names */
static int mlp_info_to_reader(DVDA_Track_Reader *r, const dvda_mlp_stream_info *info, int present)
{
    static const unsigned ident[6] = {0, 0x00, 0x01, 0x02, 0x03, 0x06};
    r->bps_code[0] = info->group0_bps;
    r->bps_code[1] = info->group1_bps;
    r->rate_code[0] = info->group0_rate;
    r->rate_code[1] = info->group1_rate;
    r->assignment = info->assignment;
    if (present && info->substreams == 2 && info->channels >= 1 && info->channels <= 5)
        r->assignment = ident[info->channels];
    r->channels = channels_of(r->assignment);
    r->interleaved = 1;            /* decoded frame-major: dvda_read() copies frames straight out */
    return r->channels != 0 && r->channels == info->channels;
}

/* ... and from the 9-byte parameter block of a raw-PCM packet: first_audio_frame 16u, 8p, bps 4u 4u, rate 4u 4u, 8p,
 * assignment 8u, 8p, crc 8u (src/pcm.c:80-96); 0 = parameters this library does not decode */
static int pcm_params_to_reader(DVDA_Track_Reader *r, const uint8_t *params, unsigned *bits, unsigned *rate)
{
    r->bps_code[0] = params[3] >> 4;
    r->bps_code[1] = params[3] & 15;
    r->rate_code[0] = params[4] >> 4;
    r->rate_code[1] = params[4] & 15;
    r->assignment = params[6];
    r->channels = channels_of(r->assignment);
    *bits = bits_of(r->bps_code[0]);
    *rate = rate_of(r->rate_code[0]);
    return r->channels && (*bits == 16 || *bits == 24) && *rate;
}

/* write_signed of one value at `bits` (src/bitstream.c:2846-2857), little-endian, `bits` / 8 bytes */
static void pack_value(uint8_t *dst, int32_t v, unsigned bits)
{
    const uint32_t sign = 1u << (bits - 1);
    const uint32_t u = ((uint32_t)v & (sign - 1)) | (v < 0 ? sign : 0u);
    for (unsigned b = 0; b < bits / 8; b++)
        dst[b] = (uint8_t)(u >> (8 * b));
}

/* ------------------------------------------------------------------ codec probe */
/* First 0xBD packet of a sector: returns 1 and its codec id, pad_2 size and the bytes behind the
 * 4-byte audio header; 0 = no audio packet in this sector; -1 = malformed (src/packet.c:61-188,
 * src/dvd-audio.c:1238-1248). */
static int first_audio_packet(const uint8_t *p, unsigned *codec, unsigned *pad2, const uint8_t **body,
                              unsigned *body_len)
{
    if (p[0] != 0 || p[1] != 0 || p[2] != 1 || p[3] != 0xBA)
        return -1;
    if ((p[4] >> 6) != 1 || !(p[4] & 4) || !(p[6] & 4) || !(p[8] & 4) || !(p[9] & 1) || (p[12] & 3) != 3)
        return -1;
    unsigned pos = 14 + (p[13] & 7);
    while (pos + 6 <= SECTOR) {
        const unsigned id = p[pos + 3], len = be16(p + pos + 4);
        if (p[pos] != 0 || p[pos + 1] != 0 || p[pos + 2] != 1 || pos + 6 + len > SECTOR)
            return -1;
        if (id == 0xBD) {
            const uint8_t *q = p + pos + 6;
            if (len < 3 || len < 7u + q[2])
                return -1;
            const unsigned pad1 = q[2];
            *codec = q[3 + pad1];
            *pad2 = q[6 + pad1];
            *body = q + 7 + pad1;
            *body_len = len - 7 - pad1;
            return 1;
        }
        pos += 6 + len;
    }
    return 0;
}

/* ------------------------------------------------------------------ device helpers */
/* DVDA_DISC_TIMING=1: where opening an MLP track spends its time, on stderr (tools/disc_bench.py; diagnostic) */
static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static int disc_timing(void)
{
    static int on = -1;
    if (on < 0)
        on = getenv("DVDA_DISC_TIMING") != NULL;
    return on;
}
static void t_line(double *t_mark, const char *what)
{
    if (t_mark && disc_timing()) {
        (void)hipDeviceSynchronize();
        const double t = now_ms();
        fprintf(stderr, "  [disc] %-28s %8.2f ms\n", what, t - *t_mark);
        *t_mark = t;
    }
}

static int dev_alloc(void **p, size_t bytes)
{
    *p = NULL;
    return hipMalloc(p, bytes ? bytes : 16) == hipSuccess;
}

/* One block on the device for the calls of a pass or of several: a host struct -- the head: descriptors, parameters,
 * results -- and `more` bytes behind it, the passes' workspace first.  Open allocates the block at *d and copies the head
 * up; DEV_AT is where a member of the head lies on the device; close copies the head back down where the calls between
 * the two went well (`ok`), and frees the block.  1 = ok. */
#define DEV_AT(d, head, member) ((void *)((d) + offsetof(__typeof__(head), member)))

static int dev_block_open(uint8_t **d, const void *head, size_t head_bytes, size_t more)
{
    return dev_alloc((void **)d, head_bytes + more) && hipMemcpy(*d, head, head_bytes, hipMemcpyHostToDevice) == hipSuccess;
}

static int dev_block_close(uint8_t *d, void *head, size_t head_bytes, int ok)
{
    ok = ok && hipMemcpy(head, d, head_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    return ok;
}

/* offset of the first major-sync pattern (bytes +4..+7 = F8 72 6F BB) at or after `from` whose
 * 8 bytes lie inside [0, size), or -1 (find_major_sync, src/dvd-audio.c:1250-1285) */
static int64_t find_sync(const uint8_t *b, uint64_t from, uint64_t size)
{
    for (uint64_t p = from; p + 8 <= size; p++)
        if (b[p + 4] == 0xF8 && b[p + 5] == 0x72 && b[p + 6] == 0x6F && b[p + 7] == 0xBB)
            return (int64_t)p;
    return -1;
}

/* the same search over device memory: windows of the payload are copied back until the pattern
 * shows up (each window overlaps the previous one by 7 bytes) */
static int64_t find_sync_dev(const uint8_t *d_bytes, uint64_t from, uint64_t size)
{
    enum { WINDOW = 1 << 16 };
    uint8_t *w = malloc(WINDOW);
    int64_t at = -1;
    if (!w)
        return -1;
    while (from + 8 <= size) {
        const uint64_t n = size - from < WINDOW ? size - from : WINDOW;
        if (hipMemcpy(w, d_bytes + from, n, hipMemcpyDeviceToHost) != hipSuccess)
            break;
        const int64_t p = find_sync(w, 0, n);
        if (p >= 0) {
            at = (int64_t)from + p;
            break;
        }
        if (n < WINDOW)
            break;
        from += n - 7;
    }
    free(w);
    return at;
}

/* The reports a reader wants (`have`: states > 0) of one piece of PCM where it lies on the device, into `out` (which may
 * be `have`): `frames` frames of `ch` channels at `bits` in `layout` at d_pcm, capacity `stride` frames.  Which of them
 * this reader has is decided here and nowhere else: a digest at 16 and 24 bits, a level report at 16, 20 and 24 bits of
 * int32 PCM, an energy report of int32 PCM at a block length the report takes -- a reader that hands out the WAV payload
 * (wav_payload) has neither of the two.  `before`: the track's frames in front of the piece: the energy report's grid is
 * the track's, so the piece's first block has what is left of the block the track is in.  One block on the device
 * (dev_block) holds the head -- the descriptor, the results, the energy report's lead and counts -- and the workspace, the
 * largest one where several reports run: they run one behind the other; the energy report's blocks lie behind it.
 * A reader that reduces the word length (have->rq > 0, bits at least its bits_out) does so HERE, first: the piece's int32
 * PCM is requantized in place from `bits` to bits_out with frame0 = `before`, so a track read whole and read in windows
 * is the same bytes, and every report behind it -- and every copy or pack the caller makes after this call -- sees the
 * PCM the reader hands out, at bits_out.
 * Blocks; what it allocates it frees; allocates and launches nothing when there is nothing to make.  1 = ok. */
static int piece_reports(struct pcm_reports *have, struct pcm_reports *out, int wav_payload, const int32_t *d_pcm,
                         uint32_t layout, unsigned bits, uint64_t stride, uint64_t frames, unsigned ch, uint64_t before)
{
    const dvda_pcm_crc_desc desc = {0, stride, frames, ch, 0};
    uint8_t *d = NULL;
    if (have->rq > 0 && bits < have->rq_par.bits_out)
        have->rq = 0;
    out->rq = have->rq;
    out->rq_par = have->rq_par;
    memset(&out->rq_rep, 0, sizeof(out->rq_rep));
    if (have->rq > 0) {
        struct {
            dvda_pcm_crc_desc desc;
            uint64_t frame0;
            dvda_pcm_requant_report rep;
        } rq = {desc, before, {0, {0}}};
        dvda_pcm_requant par = have->rq_par;
        const size_t rq_words = dvda_pcm_hip_requantize_workspace_words(1, frames);
        par.bits_in = bits;
        if (frames) {
            const int done = dev_block_open(&d, &rq, sizeof(rq), rq_words * sizeof(uint32_t)) &&
                             dvda_pcm_hip_requantize(d_pcm, layout, DEV_AT(d, rq, desc), (int32_t *)d_pcm, layout,
                                                     DEV_AT(d, rq, desc), DEV_AT(d, rq, frame0), 1, &par, frames,
                                                     DEV_AT(d, rq, rep), (uint32_t *)(d + sizeof(rq)), rq_words,
                                                     NULL) == DVDA_HIP_OK;
            if (!dev_block_close(d, &rq, sizeof(rq), done))
                return 0;
            out->rq_rep = rq.rep;
        }
        bits = have->rq_par.bits_out;
    }
    const uint64_t payload = frames * ch * (bits / 8);
    if (have->dg > 0 && bits != 16 && bits != 24)
        have->dg = -1;
    if (have->lv > 0 && (wav_payload || (bits != 16 && bits != 20 && bits != 24)))
        have->lv = -1;
    if (have->ng > 0 && (wav_payload || have->ng_block < DVDA_NRG_MIN_BLOCK || have->ng_block > DVDA_NRG_MAX_BLOCK))
        have->ng = -1;
    const int dg = have->dg > 0, lv = have->lv > 0, ng = have->ng > 0;
    const size_t w_dg = dg ? dvda_pcm_hip_crc32_workspace_words(1, payload) : 0;
    const size_t w_lv = lv ? dvda_pcm_hip_levels_workspace_words(1, frames) : 0;
    const uint32_t nrg_b = have->ng_block;
    const size_t w_ng = ng ? dvda_pcm_hip_energy_workspace_words(1, frames, nrg_b) : 0;
    const size_t w_two = w_dg > w_lv ? w_dg : w_lv;
    const size_t words = w_two > w_ng ? w_two : w_ng;
    /* the energy report: its lead (the kernels read the low word), off, cap, nblocks; its blocks lie behind the workspace */
    const uint32_t lead = ng ? nrg_b - (uint32_t)(before % nrg_b) : 0;
    const uint64_t ng_n = !ng || !frames ? 0 : 1 + ((frames > lead ? frames - lead : 0) + nrg_b - 1) / nrg_b;
    struct {
        dvda_pcm_crc_desc desc;
        uint64_t bytes;
        uint32_t crc, pad;
        dvda_pcm_levels levels;
        uint64_t ng_lead, ng_off, ng_cap, ng_got;
    } res = {desc, 0, 0, 0, {0}, lead, 0, ng_n, 0};
    const size_t ng_at = (words * sizeof(uint32_t) + 7) & ~(size_t)7;
    dvda_pcm_energy_block *ng_blocks = NULL;
    out->dg = have->dg;
    out->lv = have->lv;
    out->ng = have->ng;
    out->ng_block = nrg_b;
    out->crc = 0;
    out->bytes = 0;
    memset(&out->levels, 0, sizeof(out->levels));
    free(out->ng_blocks);
    out->ng_blocks = NULL;
    out->ng_n = out->ng_cap = 0;
    if (!frames || !words)
        return 1;                                /* (the reports of no frames are zeros, and no blocks) */
    if (ng && (ng_blocks = malloc((size_t)ng_n * sizeof(*ng_blocks))) == NULL)
        return 0;
    int ok = dev_block_open(&d, &res, sizeof(res), ng ? ng_at + (size_t)ng_n * sizeof(*ng_blocks) : words * sizeof(uint32_t));
    uint32_t *d_work = (uint32_t *)(d + sizeof(res));
    dvda_pcm_energy_block *d_blocks = (dvda_pcm_energy_block *)((uint8_t *)d_work + ng_at);     /* (only where it runs) */
    ok = ok &&
         (!dg || dvda_pcm_hip_crc32(d_pcm, layout, bits, DEV_AT(d, res, desc), 1, payload, DEV_AT(d, res, crc),
                                    DEV_AT(d, res, bytes), d_work, words, NULL) == DVDA_HIP_OK) &&
         (!lv || dvda_pcm_hip_levels(d_pcm, layout, bits, DEV_AT(d, res, desc), 1, frames, DEV_AT(d, res, levels), d_work,
                                     words, NULL) == DVDA_HIP_OK) &&
         (!ng || (dvda_pcm_hip_energy(d_pcm, layout, DEV_AT(d, res, desc), 1, nrg_b, DEV_AT(d, res, ng_lead), frames, d_blocks,
                                      DEV_AT(d, res, ng_off), DEV_AT(d, res, ng_cap), DEV_AT(d, res, ng_got), d_work, words,
                                      NULL) == DVDA_HIP_OK &&
                  hipMemcpy(ng_blocks, d_blocks, (size_t)ng_n * sizeof(*ng_blocks), hipMemcpyDeviceToHost) == hipSuccess));
    ok = dev_block_close(d, &res, sizeof(res), ok) && (!ng || res.ng_got == ng_n);
    if (ok && ng) {
        out->ng_blocks = ng_blocks;
        out->ng_n = out->ng_cap = ng_n;
    } else {
        free(ng_blocks);
    }
    if (ok) {                                    /* (zeros where a report did not run) */
        out->crc = res.crc;
        out->bytes = res.bytes;
        out->levels = res.levels;
    }
    return ok;
}

/* a piece is handed out: its reports join the track's */
static void reports_join(struct pcm_reports *track, const struct pcm_reports *piece)
{
    if (track->dg > 0) {
        track->crc = dvda_pcm_hip_crc32_combine(track->crc, piece->crc, piece->bytes);
        track->bytes += piece->bytes;
    }
    if (track->lv > 0)
        dvda_pcm_hip_levels_combine(&track->levels, &piece->levels, &track->levels);
    if (track->rq > 0) {
        track->rq_rep.frames += piece->rq_rep.frames;
        for (int c = 0; c < 8; c++)
            track->rq_rep.clipped[c] += piece->rq_rep.clipped[c];
    }
    if (track->ng > 0 && piece->ng_n) {
        /* (a piece that cannot be joined leaves a reader without the report: -1, as for one that was never made) */
        if (track->ng_n + piece->ng_n > track->ng_cap) {
            const uint64_t cap = 2 * (track->ng_n + piece->ng_n);
            dvda_pcm_energy_block *g = realloc(track->ng_blocks, (size_t)cap * sizeof(*g));
            if (g) {
                track->ng_blocks = g;
                track->ng_cap = cap;
            }
        }
        if (dvda_pcm_hip_energy_append(track->ng_blocks, &track->ng_n, track->ng_cap, piece->ng_blocks, piece->ng_n,
                                       track->ng_block) != DVDA_HIP_OK)
            track->ng = -1;
    }
}

/* What a writer is to track_write: its call on one stream -- where the PCM, the descriptors, the pass's extra record,
 * its report and its workspace lie on the device -- with the pass's own parameter, and what it keeps in the block. */
struct track_dev {
    const int32_t *in;
    int32_t *out;
    uint32_t layout;
    unsigned bits;
    const dvda_pcm_crc_desc *desc_in, *desc_out;
    const void *extra;
    void *rep;
    uint32_t *work;
    size_t words;
    uint64_t out_frames;
};
struct track_pass {
    int (*call)(const struct track_dev *v, unsigned arg);
    unsigned arg;                   /* the pass's parameter (the ratio) */
    const void *extra;              /* a record the pass reads on the device (the matrix), extra_bytes of it; or none */
    size_t extra_bytes;
    void *rep;                      /* its report, rep_bytes of it, the output's frame count frames_at bytes into it */
    size_t rep_bytes, frames_at;
    size_t words;                   /* its workspace */
};

static int call_decimate(const struct track_dev *v, unsigned ratio)
{
    return dvda_pcm_hip_decimate(v->in, v->layout, v->desc_in, v->out, v->layout, v->desc_out, NULL, 1, ratio, v->bits,
                                 v->out_frames, v->rep, v->work, v->words, NULL);
}

static int call_resample(const struct track_dev *v, unsigned none)
{
    (void)none;
    return dvda_pcm_hip_resample(v->in, v->layout, v->desc_in, v->out, v->layout, v->desc_out, NULL, 1, v->bits, v->out_frames,
                                 v->rep, v->work, v->words, NULL);
}

static int call_mix(const struct track_dev *v, unsigned none)
{
    (void)none;
    return dvda_pcm_hip_mix(v->in, v->layout, v->desc_in, v->out, v->layout, v->desc_out, v->extra, 1, v->bits, v->out_frames,
                            v->rep, v->work, v->words, NULL);
}

/* A whole track through a writer where it lies on the device: `frames` frames of `ch` channels at `bits` in `layout` (an
 * int32 one) at *d_pcm, capacity *stride frames, go as one whole track (no piece) through p->call into a second buffer in
 * the same layout -- out_frames frames of out_ch channels, the stride padded to a multiple of 4 -- which takes the place
 * of the first: *d_pcm and *stride are then those of the track the pass made, and everything the reader does from here on
 * sees that track.  One block on the device holds the two descriptors, the pass's extra record, its report and its
 * workspace.  The pass must report out_frames frames (no frames: no call, a report of zeros).  Blocks; the first buffer
 * is freed.  1 = ok. */
static int track_write(int32_t **d_pcm, uint32_t layout, unsigned bits, uint64_t *stride, uint64_t frames, unsigned ch,
                       uint64_t out_frames, unsigned out_ch, const struct track_pass *p)
{
    uint64_t out_stride = (out_frames + 3) & ~(uint64_t)3;
    if (out_stride == 0)
        out_stride = 4;
    const dvda_pcm_crc_desc desc[2] = {{0, *stride, frames, ch, 0}, {0, out_stride, out_frames, out_ch, 0}};
    /* the head: the descriptors | the extra record | the report (room for the largest of either) */
    uint8_t head[sizeof(desc) + sizeof(dvda_pcm_mix) + sizeof(dvda_pcm_decim_report)];
    const size_t rep_at = sizeof(desc) + p->extra_bytes, head_bytes = rep_at + p->rep_bytes;
    if (head_bytes > sizeof(head))
        return 0;
    memset(head, 0, sizeof(head));
    memcpy(head, desc, sizeof(desc));
    if (p->extra_bytes)
        memcpy(head + sizeof(desc), p->extra, p->extra_bytes);
    int32_t *d_out = NULL;
    uint8_t *d = NULL;
    int ok = dev_alloc((void **)&d_out, (size_t)out_stride * out_ch * sizeof(int32_t));
    if (ok && out_frames) {
        uint64_t made = 0;
        ok = dev_block_open(&d, head, head_bytes, p->words * sizeof(uint32_t));
        if (ok) {
            const struct track_dev v = {*d_pcm, d_out, layout, bits, (const dvda_pcm_crc_desc *)d,
                                        (const dvda_pcm_crc_desc *)d + 1, d + sizeof(desc), d + rep_at,
                                        (uint32_t *)(d + head_bytes), p->words, out_frames};
            ok = p->call(&v, p->arg) == DVDA_HIP_OK;
        }
        ok = dev_block_close(d, head, head_bytes, ok);
        memcpy(&made, head + rep_at + p->frames_at, sizeof(made));
        ok = ok && made == out_frames;
    }
    if (!ok) {
        (void)hipFree(d_out);
        return 0;
    }
    (void)hipFree(*d_pcm);
    *d_pcm = d_out;
    *stride = out_stride;
    memcpy(p->rep, head + rep_at, p->rep_bytes);
    return 1;
}

/* dvda_hip_set_decimate, and with ratio 0 dvda_hip_set_resample (48 kHz to 44.1 kHz): *frames is then the frame count of
 * the track at the lower rate */
static int track_decimate(int32_t **d_pcm, uint32_t layout, unsigned bits, uint64_t *stride, uint64_t *frames, unsigned ch,
                          unsigned ratio, dvda_pcm_decim_report *rep)
{
    const uint64_t out_frames = ratio ? dvda_pcm_hip_decim_out_frames(0, *frames, ratio)
                                      : dvda_pcm_hip_resample_out_frames(0, *frames);
    const struct track_pass p = {ratio ? call_decimate : call_resample, ratio, NULL, 0, rep, sizeof(*rep),
                                 offsetof(dvda_pcm_decim_report, frames_out),
                                 ratio ? dvda_pcm_hip_decimate_workspace_words(1, out_frames)
                                       : dvda_pcm_hip_resample_workspace_words(1, out_frames)};
    if (!track_write(d_pcm, layout, bits, stride, *frames, ch, out_frames, ch, &p))
        return 0;
    *frames = out_frames;
    return 1;
}

/* dvda_hip_set_downmix: the track's *ch channels (the channels of `mask`, ascending) through the default matrix of `mask`
 * to out_ch channels; the reader is the track of out_ch channels from here on */
static int track_mix(int32_t **d_pcm, uint32_t layout, unsigned bits, uint64_t *stride, uint64_t frames, unsigned *ch,
                     unsigned mask, unsigned out_ch, unsigned flags, dvda_pcm_mix_report *rep)
{
    dvda_pcm_mix mix;
    const struct track_pass p = {call_mix, 0, &mix, sizeof(mix), rep, sizeof(*rep), offsetof(dvda_pcm_mix_report, frames),
                                 dvda_pcm_hip_mix_workspace_words(1, frames)};
    /* (a matrix the kernels would not take -- DVDA_MIX_UNITY rows above 2^31 -- or a mask of other channels: no reader) */
    if (dvda_pcm_hip_mix_matrix(mask, out_ch, flags, &mix) != DVDA_HIP_OK || !dvda_pcm_hip_mix_valid(&mix) ||
        mix.in_channels != *ch || !track_write(d_pcm, layout, bits, stride, frames, *ch, frames, out_ch, &p))
        return 0;
    *ch = out_ch;
    return 1;
}

/* What a whole-track reader, MLP or raw PCM, does with its track once it lies decoded on the device -- r->frames frames of
 * r->channels channels at the depth and rate of r's codes in `layout` at *d_pcm, capacity `stride` -- before any copy to
 * the host: FIRST the channel mix where it applies (dvda_hip_set_downmix: r->channels and r->stride are the mixed
 * track's from there on, r->src_channels the disc's), then the decimation or the resampler where they apply (from there
 * on the reader IS the shorter track at the lower rate), then the reports the options want of the track as that left
 * it, the word-length reduction among them: the reader hands out bits_out bits from there on.  Every stage rounds and
 * clamps, so this order is part of the contract.  1 = ok. */
static int track_passes(DVDA_Track_Reader *r, const struct reader_opts *o, int32_t **d_pcm, uint32_t layout, int wav_payload,
                        uint64_t stride)
{
    const unsigned bits = bits_of(r->bps_code[0]);
    r->stride = stride;
    /* the channel mix first, at the track's depth: every stage rounds and clamps, so the order is part of the contract */
    if (mx_applies(o, r->channels)) {
        const unsigned src = r->channels;
        if (!track_mix(d_pcm, layout, bits, &r->stride, r->frames, &r->channels, dvda_pcm_hip_speaker_mask(r->assignment),
                       o->mx_ch, o->mx_flags, &r->mx_rep))
            return 0;
        r->src_channels = src;
    }
    if (rs_applies(o, r->rate_code[0])) {
        /* 96 / 192 kHz: by 2 / 4 to 48 kHz at the track's depth first; then 48 kHz to 44.1 kHz into a new buffer */
        const unsigned shift = r->rate_code[0] & 3;
        if (shift) {
            if (!track_decimate(d_pcm, layout, bits, &r->stride, &r->frames, r->channels, 1u << shift, &r->dc_rep))
                return 0;
            r->dc_done = 1;
        }
        if (!track_decimate(d_pcm, layout, bits, &r->stride, &r->frames, r->channels, 0, &r->rs_rep))
            return 0;
        r->rs_done = 1;
        r->src_rate = rate_of(r->rate_code[0]);
        r->rate_code[0] = 8;            /* 44 100 Hz */
    } else if (dc_applies(o, r->rate_code[0])) {
        if (!track_decimate(d_pcm, layout, bits, &r->stride, &r->frames, r->channels, o->dc_ratio, &r->dc_rep))
            return 0;
        r->dc_done = 1;
        r->src_rate = rate_of(r->rate_code[0]);
        r->rate_code[0] -= dc_shift(o);
    }
    rep_want(&r->rep, o);
    if (!piece_reports(&r->rep, &r->rep, wav_payload, *d_pcm, layout, bits, r->stride, r->frames, r->channels, 0))
        return 0;
    if (r->rep.rq > 0) {
        r->src_bits = bits;
        r->bps_code[0] = code_of_bits(o->rq_bits);
    }
    return 1;
}

/* ------------------------------------------------------------------ the buffer set
 * Everything a track's decode works in.  The steps below fill and use it; who owns it decides how it is allocated:
 *   one batch (pinned == 0)  pageable sector buffer, device buffers of exactly the size in use, the whole set freed when
 *                            the reader has been opened (the decoded PCM moves into the reader)
 *   windows   (pinned == 1)  pinned sector buffer, buffers that are kept from window to window and grow with slack, the
 *                            whole set handed from reader to reader through the thread's cache
 */
struct track_bufs {
    dvda_mlp_hip_ctx *ctx;
    uint32_t ctx_segs;          /* segment capacity ctx was (or is to be) created with */
    uint8_t *h_sec, *d_sec;     /* sectors, host and device */
    uint8_t *d_mlp;             /* their MLP payload */
    uint32_t *d_work, *h_base;  /* workspace of the sector kernels; host: where each sector begins in the payload */
    uint8_t *d_stream;          /* the MLP stream that is indexed and decoded */
    uint64_t *d_meta;
    int32_t *d_pcm, *d_fir;
    uint8_t *carry;             /* host: stream bytes from a window's cut on */
    size_t cap_sec, cap_stream, cap_pcm, carry_cap;     /* sectors, bytes, bytes, bytes */
    int pinned;                 /* h_sec is pinned host memory */
    size_t host_now, host_peak; /* pinned and carried host bytes held through this set, window slots included (windows) */
};

static void bufs_free(struct track_bufs *b)
{
    if (b->ctx)
        dvda_mlp_hip_destroy(b->ctx);
    if (b->pinned && b->h_sec)
        (void)hipHostFree(b->h_sec);
    else
        free(b->h_sec);
    free(b->h_base);
    free(b->carry);
    (void)hipFree(b->d_sec);
    (void)hipFree(b->d_mlp);
    (void)hipFree(b->d_stream);
    (void)hipFree(b->d_work);
    (void)hipFree(b->d_meta);
    (void)hipFree(b->d_pcm);
    (void)hipFree(b->d_fir);
    memset(b, 0, sizeof(*b));
}

static void bufs_host_add(struct track_bufs *b, size_t now_more)
{
    b->host_now += now_more;
    if (b->host_now > b->host_peak)
        b->host_peak = b->host_now;
}

/* `need` bytes at *p: a set that is kept keeps what is large enough and grows with slack, the other is sized exactly */
static int bufs_dev_room(const struct track_bufs *b, void **p, size_t *cap, size_t need)
{
    if (b->pinned && need <= *cap && *p)
        return 1;
    (void)hipFree(*p);
    *p = NULL;
    *cap = 0;
    if (b->pinned)
        need += need / 4 + 4096;
    if (!dev_alloc(p, need))
        return 0;
    *cap = need;
    return 1;
}

/* device side of `n` sectors: their copy, their MLP payload (mlp), the workspace, and the host copy of the offsets */
static int bufs_sector_room(struct track_bufs *b, unsigned n, int mlp)
{
    const size_t cap = (size_t)n * SECTOR;
    if (!dev_alloc((void **)&b->d_sec, cap) || (mlp && !dev_alloc((void **)&b->d_mlp, cap + 64)) ||
        !dev_alloc((void **)&b->d_work, dvda_pcm_hip_workspace_words(n) * sizeof(uint32_t)) ||
        (b->h_base = malloc(((size_t)n + 1) * sizeof(uint32_t))) == NULL)
        return 0;
    b->cap_sec = n;
    return 1;
}

/* ------------------------------------------------------------------ the steps of a track's decode */

/* Sectors [first, first + want) of the files -> the device -> their MLP payload in d_mlp (ch == 0), or the un-swizzled
 * planes of raw PCM at `bits` and `ch` channels in d_pcm, *stride frames each.  *got = sectors read; *total = payload
 * bytes / PCM frames in them; h_base[s] = where sector s begins among those (h_base[got] = *total).  A set that holds
 * fewer than `want` sectors is grown: a pinned one for `want`, the other for what was read.  1 = done (*got may be 0:
 * nothing there to read), 0 = failure. */
static int sectors_to_device(struct track_bufs *b, struct aob_set *aobs, unsigned first, unsigned want, unsigned bits,
                             unsigned ch, double *t_mark, unsigned *got, uint64_t *total, uint64_t *stride)
{
    const int mlp = ch == 0;
    *got = 0;
    *total = 0;
    if (want > b->cap_sec) {
        if (b->pinned && b->h_sec) {
            (void)hipHostFree(b->h_sec);
            b->host_now -= b->cap_sec * SECTOR;
        } else {
            free(b->h_sec);
        }
        (void)hipFree(b->d_sec);
        if (mlp)
            (void)hipFree(b->d_mlp);
        (void)hipFree(b->d_work);
        free(b->h_base);
        b->h_sec = b->d_sec = NULL;
        if (mlp)
            b->d_mlp = NULL;
        b->d_work = b->h_base = NULL;
        b->cap_sec = 0;
        const size_t cap = (size_t)want * SECTOR;
        if (!b->pinned) {
            if ((b->h_sec = malloc(cap)) == NULL)
                return 0;
        } else {
            if (hipHostMalloc((void **)&b->h_sec, cap, hipHostMallocDefault) != hipSuccess)
                return 0;
            bufs_host_add(b, cap);
            if (!bufs_sector_room(b, want, mlp))
                return 0;
        }
    }
    const unsigned n = want ? aob_read(aobs, first, want, b->h_sec) : 0;
    if (!n)
        return 1;
    t_line(t_mark, "sectors read from the files");
    if (!b->cap_sec && !bufs_sector_room(b, n, mlp))
        return 0;
    if (!mlp) {
        /* a sector holds at most 2013 payload bytes: upper bound of the PCM frames */
        *stride = (uint64_t)n * (2013 / (ch * (bits / 8) * 2)) * 2;
        *stride = (*stride + 3) & ~(uint64_t)3;
        if (!bufs_dev_room(b, (void **)&b->d_pcm, &b->cap_pcm, *stride * ch * sizeof(int32_t)))
            return 0;
    }
    if (hipMemcpy(b->d_sec, b->h_sec, (size_t)n * SECTOR, hipMemcpyHostToDevice) != hipSuccess)
        return 0;
    if ((mlp ? dvda_mlp_hip_demux_sectors(b->d_sec, n, b->d_mlp, (size_t)b->cap_sec * SECTOR, b->d_work, NULL)
             : dvda_pcm_hip_decode_sectors(b->d_sec, n, bits, ch, b->d_pcm, *stride, b->d_work, NULL)) != DVDA_HIP_OK)
        return 0;
    /* (`bad` also counts the sectors of a following track of the other codec inside the look-ahead: they contribute
       nothing, which is what is wanted of them.  A sector with more audio packets than the kernels keep is refused by
       scan and gather alike, csrc/pcm_unswizzle.h.) */
    uint32_t bad = 0;
    if (dvda_pcm_hip_result(b->d_work, n, total, &bad, NULL) != DVDA_HIP_OK)
        return 0;
    /* workspace words [n, 2 * n]: the offset of every sector, then the total */
    if (hipMemcpy(b->h_base, b->d_work + n, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return 0;
    *got = n;
    return 1;
}

/* Where the stream of a track (or of one window of it) begins and ends in the `total` payload bytes of `got` sectors, of
 * which the first `in_track` are the track's own and the rest the look-ahead behind it (decode_mlp_audio +
 * mlp_data_to_major_sync, src/dvd-audio.c:1167-1194, 1367-1421):
 *   begin   first_sync: the first major sync, found byte by byte -- else 0, the stream runs on from the window before
 *   end     last_window == 0: all of it.  Else the first major sync at or behind the first payload byte of a sector
 *           beyond the track; all of it when the title set ends with the track; 7 bytes short of the data when packets
 *           follow but no sync does and the files end here (find_major_sync needs 8)
 * 1 = found, 0 = the look-ahead (want - in_track sectors) was too short: four times as much, -1 = no such stream. */
static int stream_bounds(const struct track_bufs *b, int first_sync, int last_window, unsigned in_track, unsigned got,
                         unsigned want, int files_end, uint64_t total, uint64_t *begin, uint64_t *end)
{
    *begin = 0;
    *end = total;
    if (first_sync) {
        const int64_t s0 = find_sync_dev(b->d_mlp, 0, total);
        if (s0 < 0)                  /* no major sync anywhere: the reference asserts */
            return (!last_window || got < want || files_end) ? -1 : 0;
        *begin = (uint64_t)s0;
    }
    if (!last_window || got <= in_track)
        return 1;
    const uint64_t boundary = b->h_base[in_track];
    const int64_t s1 = find_sync_dev(b->d_mlp, boundary > *begin ? boundary : *begin, total);
    if (s1 >= 0)
        *end = (uint64_t)s1;
    else if (files_end)
        *end = total - boundary >= 8 ? total - 7 : boundary;
    else
        return 0;
    return 1;
}

/* index of stream bytes [0, len) in d_stream; makes the context, and makes it again when it has too few segments */
static int index_stream(struct track_bufs *b, const struct reader_opts *o, uint64_t len, uint32_t *n_seg)
{
    const uint64_t padded = (len + 15) & ~(uint64_t)15;
    const uint64_t meta[4] = {0, len, 0, 0};
    if ((!b->d_meta && !dev_alloc((void **)&b->d_meta, sizeof(meta))) ||
        hipMemsetAsync(b->d_stream + len, 0, padded + 64 - len, NULL) != hipSuccess ||
        hipMemcpy(b->d_meta, meta, sizeof(meta), hipMemcpyHostToDevice) != hipSuccess)
        return 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (!b->ctx) {
            if (b->ctx_segs == 0)
                b->ctx_segs = (uint32_t)(len / 2048 + 256);
            if (dvda_mlp_hip_create(&b->ctx, o->device, 1, b->ctx_segs) != DVDA_HIP_OK)
                return 0;
        }
        /* (a context kept from the thread's last reader may have served the other presentation) */
        /* (... or conceal mode, which it does not share a context with: taken off first, put on last) */
        if (!o->conceal && dvda_mlp_hip_set_conceal(b->ctx, 0) != DVDA_HIP_OK)
            return 0;
        if (dvda_mlp_hip_set_presentation(b->ctx, o->present ? DVDA_PRESENT_SUBSTREAM0 : DVDA_PRESENT_FULL) != DVDA_HIP_OK)
            return 0;
        /* (conceal mode of the presentation: the batch tier has none and says DVDA_HIP_EINVAL -- the reader does not open) */
        if (o->conceal && dvda_mlp_hip_set_conceal(b->ctx, 1) != DVDA_HIP_OK)
            return 0;
        if (dvda_mlp_hip_index(b->ctx, b->d_stream, padded, b->d_meta + 0, b->d_meta + 1, 1, NULL) != DVDA_HIP_OK)
            return 0;
        const int rc = dvda_mlp_hip_segment_count(b->ctx, n_seg, NULL);
        if (rc == DVDA_HIP_OK)
            return 1;
        if (rc != DVDA_HIP_ECAPACITY || attempt)
            return 0;
        dvda_mlp_hip_destroy(b->ctx);
        b->ctx = NULL;
        b->ctx_segs = b->pinned ? *n_seg + *n_seg / 2 + 64 : *n_seg + 16;     /* (kept for the tracks to come / this one's) */
    }
    return 0;
}

static uint32_t layout_of(int wav_bits)
{
    return wav_bits == 24 ? DVDA_PCM_WAV24 : wav_bits == 16 ? DVDA_PCM_WAV16 : DVDA_PCM_INTERLEAVED;
}

/* Decode of the indexed stream [0, len) into d_pcm, from the FIR history `fir` (host; NULL: none).  *wav_bits < 0 asks for
 * the payload dvda2wav would write -- interleaved, little-endian, write_signed at the stream's own bit depth -- and
 * nothing else, no int32 PCM and no separate packing pass (SURVEY 8(f-3) fused into the decode, DVDA_PCM_WAV24 /
 * WAV16): decided here, from the index's stream record, as 16, 24 or 0 (a depth that is decoded into int32 frames) and
 * then left alone; a reader that reduces the word length or decimates (rq: its options, or NULL) decodes int32 frames,
 * which those passes work on: 0.  Hands back the stream's record after the decode and the frames d_pcm has room for.  Its status is
 * the caller's to judge.  1 = decoded, 0 = failure. */
static int decode_stream(struct track_bufs *b, uint64_t len, const int32_t *fir, int *wav_bits,
                         dvda_mlp_stream_info *info, uint64_t *stride_out, const struct reader_opts *rq)
{
    if (dvda_mlp_hip_stream_info(b->ctx, info, 1, NULL) != DVDA_HIP_OK || info->channels == 0)
        return 0;
    if (fir && ((!b->d_fir && !dev_alloc((void **)&b->d_fir, 2 * 48 * sizeof(int32_t))) ||
                hipMemcpy(b->d_fir, fir, 2 * 48 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess))
        return 0;
    if (dvda_mlp_hip_set_initial_fir(b->ctx, fir ? b->d_fir : NULL) != DVDA_HIP_OK)
        return 0;
    const unsigned rate = rate_of(info->group0_rate);
    const uint64_t per_au = rate == 48000 || rate == 44100 ? 40 : rate == 96000 || rate == 88200 ? 80 : 160;
    uint64_t stride = (info->mlp_frames * per_au + 3) & ~(uint64_t)3;
    if (stride == 0)
        stride = 4;
    if (*wav_bits < 0) {
        const unsigned bits = bits_of(info->group0_bps);
        *wav_bits = (bits == 16 || bits == 24) && !(rq && (rq_applies(rq, bits) || dc_applies(rq, info->group0_rate) ||
                                                           rs_applies(rq, info->group0_rate) || mx_applies(rq, info->channels)))
                        ? (int)bits : 0;
    }
    const unsigned wbits = (unsigned)*wav_bits;
    if (dvda_mlp_hip_set_pcm_layout(b->ctx, layout_of(*wav_bits)) != DVDA_HIP_OK)
        return 0;
    for (int attempt = 0;; attempt++) {
        const uint64_t meta[4] = {0, len, 0, stride};
        /* (as packed bytes the track takes 3/4 or 1/2 of the int32 words; the buffer is sized in int32 words either
         *  way: the decode's offsets are in those units) */
        const uint64_t words = wbits ? (stride * info->channels * (wbits / 8) + 3) / 4 + 4 : stride * info->channels;
        if (!bufs_dev_room(b, (void **)&b->d_pcm, &b->cap_pcm, words * sizeof(int32_t)) ||
            hipMemcpy(b->d_meta, meta, sizeof(meta), hipMemcpyHostToDevice) != hipSuccess)
            return 0;
        if (dvda_mlp_hip_decode(b->ctx, b->d_pcm, b->d_meta + 2, b->d_meta + 3, NULL) != DVDA_HIP_OK ||
            dvda_mlp_hip_stream_info(b->ctx, info, 1, NULL) != DVDA_HIP_OK)
            return 0;
        if (!(info->status & DVDA_ST_OVERFLOW))
            break;
        /* access units longer than the standard length: pcm_frames is the size needed */
        if (attempt)
            return 0;
        stride = (info->pcm_frames + 3) & ~(uint64_t)3;
    }
    *stride_out = stride;
    return 1;
}

/* How many of the `total` PCM frames of `got` sectors a raw-PCM track takes, `done` of its `want` frames delivered
 * before them: whole packets until the length is covered, the opening packet regardless (open_pcm_track_reader /
 * decode_pcm_audio, src/dvd-audio.c:958-1084).  *covered = the track ends inside these sectors. */
static uint64_t pcm_deliver(const uint32_t *h_base, unsigned got, uint64_t total, uint64_t done, uint64_t want, int *covered)
{
    *covered = 1;
    if (want == 0)
        return h_base[1] < total ? h_base[1] : total;
    for (unsigned s = 0; s < got; s++)
        if (done + h_base[s + 1] >= want)
            return h_base[s + 1];
    *covered = 0;
    return total;
}

static void windows_free(struct track_windows *w);

static void reader_free(DVDA_Track_Reader *r)
{
    if (!r)
        return;
    windows_free(r->win);
    free(r->pcm);
    (void)hipFree(r->d_wav);
    free(r->wav);
    free(r->spans);
    free(r->rep.ng_blocks);
    if (r->d_pcm)
        (void)hipFree(r->d_pcm);
    free(r);
}

/* ------------------------------------------------------------------ MLP track, as one batch */
static DVDA_Track_Reader *open_mlp(struct aob_set *aobs, const DVDA_Track *k, const struct reader_opts *o)
{
    DVDA_Track_Reader *r = NULL;
    struct track_bufs b;
    const unsigned first = k->s.first;
    const unsigned in_track = k->s.last >= first ? k->s.last - first + 1 : 1;
    unsigned got = 0;
    uint64_t total = 0, begin = 0, end = 0, stride = 0;
    uint32_t n_seg = 0;
    int wav_bits = o->wav_output ? -1 : 0;
    dvda_mlp_stream_info info;
    double t_mark = now_ms();

    memset(&b, 0, sizeof(b));
    /* sectors of the track plus a few behind it: the stream runs on to the next major sync */
    for (unsigned extra = 8;; extra *= 4) {
        unsigned want = in_track + extra;
        if (first + want > aobs->total || first + want < first)
            want = aobs->total - first;
        bufs_free(&b);
        if (!sectors_to_device(&b, aobs, first, want, 0, 0, &t_mark, &got, &total, NULL) || !got)
            goto out;
        t_line(&t_mark, "to the device + demux");
        const int rc = stream_bounds(&b, 1, 1, in_track, got, want, first + got >= aobs->total, total, &begin, &end);
        if (rc < 0)
            goto out;
        if (rc)
            break;
    }
    if (end <= begin)
        goto out;
    t_line(&t_mark, "major syncs at both ends");
    const uint64_t len = end - begin;
    if (!dev_alloc((void **)&b.d_stream, ((len + 15) & ~(uint64_t)15) + 64) ||
        hipMemcpy(b.d_stream, b.d_mlp + begin, len, hipMemcpyDeviceToDevice) != hipSuccess)
        goto out;
    (void)hipFree(b.d_sec);
    (void)hipFree(b.d_mlp);
    b.d_sec = b.d_mlp = NULL;
    if (!index_stream(&b, o, len, &n_seg))
        goto out;
    t_line(&t_mark, "context + index");
    if (!decode_stream(&b, len, NULL, &wav_bits, &info, &stride, o))
        goto out;
    t_line(&t_mark, "decode");
    /* the reference assert()s on a damaged stream; conceal mode hands it out composed (DVDA_ST_CONCEALED) */
    if (info.status & ~(uint32_t)(DVDA_ST_BENIGN | (o->conceal ? DVDA_ST_CONCEALED : 0u)))
        goto out;
    r = calloc(1, sizeof(*r));
    if (!r)
        goto out;
    if (info.status & DVDA_ST_CONCEALED) {
        /* the stream is the track's: the batch tier's spans are in track terms as they are */
        uint32_t n = 0;
        if (dvda_mlp_hip_conceal_spans(b.ctx, 0, NULL, 0, &n, NULL) != DVDA_HIP_OK ||
            (r->spans = malloc((n ? n : 1) * sizeof(*r->spans))) == NULL ||
            dvda_mlp_hip_conceal_spans(b.ctx, 0, r->spans, n, &n, NULL) != DVDA_HIP_OK)
            goto fail;
        r->n_spans = n;
    }
    r->codec = DVDA_MLP;
    r->status = info.status;
    r->frames = info.pcm_frames;
    if (!mlp_info_to_reader(r, &info, o->present))
        goto fail;
    /* (a track that is decimated has int32 PCM: decode_stream saw the option) */
    if ((wav_bits && (dc_applies(o, info.group0_rate) || rs_applies(o, info.group0_rate) || mx_applies(o, r->channels))) ||
        !track_passes(r, o, &b.d_pcm, layout_of(wav_bits), wav_bits != 0, stride))
        goto fail;
    if (r->src_rate || r->src_channels) {
        b.cap_pcm = 0;          /* (b.d_pcm is the decimation's buffer, or the mix's) */
        t_line(&t_mark, "decimate + reports");
    }
    if (wav_bits) {
        r->d_wav = (uint8_t *)b.d_pcm;
        r->wav_bytes = r->frames * r->channels * ((unsigned)wav_bits / 8);
    } else {
        r->d_pcm = b.d_pcm;            /* the host copy is made by the first dvda_read() */
    }
    b.d_pcm = NULL;
    goto out;
fail:
    reader_free(r);
    r = NULL;
out:
    bufs_free(&b);
    return r;
}

/* ------------------------------------------------------------------ MLP track, in windows (round 5)
 *
 * The reference streams a track of any length in O(packet) memory (src/dvd-audio.c:751-795, 1151-1227).  open_mlp()
 * above takes the whole track as ONE batch -- its sectors, its bytes and its PCM all resident at once: a 74-minute
 * 6-channel track is ~10 GB on the device and again on the host.  A track of more than WINDOW_SECTORS sectors is
 * therefore read and decoded window by window:
 *
 *   window = the next WINDOW_SECTORS sectors of the track -> GPU demux -> [bytes kept from the window before | new bytes]
 *   cut    = the LAST major sync of that stream at which a segment starts AND every substream restarts
 *            (win_unit_restarts: a window cannot begin at a sync that restarts nothing) (the index says where: restart segments
 *            are the units of parallel decode): everything in front of it is whole segments and is decoded
 *            now; what follows is kept for the next window.  The first window starts at the first major-sync
 *            pattern, the last one ends as open_mlp()'s whole track does (src/dvd-audio.c:1167-1194).
 *   carry  = between two windows nothing but those bytes and the FIR history at the cut (the reference never clears a
 *            channel's history, src/mlp.c:297-304: dvda_mlp_hip_segment_fir / dvda_mlp_hip_set_initial_fir) -- every
 *            other decoder field is set again by the restart header at a major sync.
 *
 * A producer thread fills a ring of two pinned host buffers (window k + 1 is read, demultiplexed and decoded while
 * dvda_read() / dvda_hip_reader_wav_next() serve window k); one decode context, one set of device buffers and the two
 * pinned buffers serve the whole track.  What is resident is bounded by the window, not by the track:
 * dvda_hip_reader_memory() reports the peaks (tests/test_disc_api.py asserts them).
 */
#define WIN_SLOTS 2
static unsigned window_sectors(void)
{
    /* DVDA_WINDOW_SECTORS: window size in 2048-byte sectors (tests use small ones); default 8192 = 16 MiB of sectors,
       which decode to 32..70 MB of PCM */
    const char *e = getenv("DVDA_WINDOW_SECTORS");
    const long v = e ? strtol(e, NULL, 10) : 0;
    return v >= 64 ? (unsigned)v : 8192u;
}

struct win_slot {
    uint8_t *host;              /* pinned: int32 frames [frame][channel], or the packed WAV payload */
    size_t cap;
    uint64_t frames;
    uint64_t stride;            /* != 0: int32 PLANAR [channel][stride] (raw-PCM windows: the order the un-swizzle writes) */
    struct pcm_reports rep;     /* of the window, made on the device before it was copied */
};

struct track_windows {
    struct aob_set aobs;        /* the reader's own open files */
    unsigned last;              /* the track's last sector */
    unsigned next;              /* next sector to read */
    unsigned window;
    int (*produce)(struct track_windows *, struct win_slot *);      /* win_produce or win_produce_pcm */
    struct reader_opts opts;    /* what the reader was opened with */
    int wav_bits;               /* != 0: the windows hold the payload (DVDA_PCM_WAV24 / WAV16); < 0 until the first
                                   window's major sync has decided it: only a 16- or 24-bit stream is decoded straight
                                   into it */
    uint64_t rep_before;        /* the track's frames that went through piece_reports() so far (the producing thread's) */
    struct pcm_reports rep;     /* states: what every window is asked on the device before it is copied (-1: decided by the
                                   first window's piece_reports()); values: the windows handed out so far, joined (under
                                   `mu`, win_release()) */
    int started, finished, failed;
    /* a raw-PCM track read in windows (round 6): sectors decode independently of each other (src/pcm.c:149: whole chunks
       per packet), so a window is a run of sectors and nothing crosses a cut but the count of frames delivered so far */
    unsigned pcm_bits, pcm_channels;
    unsigned pcm_out_bits;      /* the depth the reader hands out: pcm_bits, or what the word-length reduction leaves */
    uint64_t pcm_want;          /* the track's length in PCM frames (its PTS length); whole packets until it is covered */
    uint64_t pcm_done;
    uint8_t *pack_tmp;          /* host: a planar window packed for dvda_hip_reader_wav_next() on an int32 reader */
    size_t pack_cap;
    size_t carry_len;           /* bytes of b.carry in use: the stream from the last cut on */
    int32_t fir[2 * 48];
    int have_fir;
    struct track_bufs b;        /* kept for the whole track, and in the thread's cache for the next one */
    /* conceal mode (opts.conceal): every window is a conceal-mode stream of its own; what lies between two of them is
       stitched here (win_conceal_stitch).  Private to the producing thread but for `spans`. */
    struct {
        int have_edge;          /* a window so far kept something: t_end is the input timing behind its last kept unit */
        uint32_t t_end, cause;  /* ... and the causes of the damage since */
        uint64_t B;             /* stream bytes since: the tail behind kept_end, windows that kept nothing, the bytes in
                                   front of the next kept_begin */
        uint64_t pend_off;      /* track offset where those bytes begin */
        uint64_t kept_bytes, kept_frames;       /* over the track so far: the running mean of the gap rule */
        uint64_t base;          /* track offset of d_stream[0] */
        uint64_t frames;        /* PCM frames decided so far, silence included */
        uint64_t sil_left;      /* frames of silence still to hand out in front of the held window */
        int held, held_final;   /* b.d_pcm holds a decoded window that waits behind that silence */
        dvda_mlp_stream_info held_info;
        uint64_t held_stride;
        int32_t *d_zero;        /* device: one silent window of bounded size */
        dvda_mlp_conceal_span *p_spans;         /* spans made since the last win_commit() */
        unsigned p_n, p_cap;
    } cw;
    dvda_mlp_conceal_span *spans;       /* published under `mu` (win_commit) */
    unsigned n_spans, cap_spans;
    /* what the stream is (first window) */
    dvda_mlp_stream_info info;
    unsigned status;            /* (with frames_total and `finished`: published under `mu`, win_commit()) */
    uint64_t frames_total;
    /* what produce() found, private to the thread that runs it until win_commit() publishes it under `mu` -- in the
       same critical section that queues the window (round 6: `finished` used to be set by win_produce itself, without
       the lock, BEFORE the producer queued the last window: a consumer that looked in between saw "no window, finished"
       and reported the end of the track with the last window still unqueued) */
    int p_final;
    unsigned p_status;
    uint64_t p_frames;
    /* producer / consumer */
    pthread_t th;
    int th_started, stop;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    struct win_slot slot[WIN_SLOTS];
    unsigned head, tail, count;
    uint64_t served_in_slot;    /* frames of slot[tail] already handed out */
    uint8_t *whole;             /* dvda_hip_reader_wav_payload() on a windowed reader: every window appended (unbounded) */
    /* accounting (the host side: b.host_now / b.host_peak) */
    size_t dev_free0, dev_peak;
    size_t dev_base;            /* device memory the reader took over from the thread's cache (already allocated at dev_free0) */
};

static void win_dev_sample(struct track_windows *w)
{
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && w->dev_free0 > fr && w->dev_base + (w->dev_free0 - fr) > w->dev_peak)
        w->dev_peak = w->dev_base + (w->dev_free0 - fr);
}

/* room for `bytes` in a pinned window slot */
static int slot_reserve(struct track_bufs *b, struct win_slot *s, size_t bytes)
{
    if (bytes <= s->cap)
        return 1;
    if (s->host) {
        (void)hipHostFree(s->host);
        b->host_now -= s->cap;
    }
    s->host = NULL;
    s->cap = bytes + bytes / 4 + 4096;
    if (hipHostMalloc((void **)&s->host, s->cap, hipHostMallocDefault) != hipSuccess) {
        s->cap = 0;
        return 0;
    }
    bufs_host_add(b, s->cap);
    return 1;
}

/* What a windowed reader allocated -- its buffer set (the decode context, the device buffers, the pinned sector buffer)
 * and the window slots -- kept by the thread that closes it for the next windowed reader the same thread opens on the
 * same device (round 5: a worker of dvda2wav_hip extracts track after track; allocating and freeing all of it was 50 of
 * a track's 90 ms, tools/probe/r05_disc_time.sh).  One set per thread; dvda_hip_release_cached_buffers() frees the
 * caller's. */
struct win_cache {
    struct track_bufs b;
    int valid, device;
    struct win_slot slot[WIN_SLOTS];
    size_t dev_bytes;           /* device memory the set took at its reader's peak (the host side: b.host_now) */
};
static __thread struct win_cache t_win_cache;

static void win_cache_free(struct win_cache *c)
{
    if (!c->valid)
        return;
    (void)hipSetDevice(c->device);
    bufs_free(&c->b);
    for (int i = 0; i < WIN_SLOTS; i++)
        if (c->slot[i].host)
            (void)hipHostFree(c->slot[i].host);
    memset(c, 0, sizeof(*c));
}

void dvda_hip_release_cached_buffers(void) { win_cache_free(&t_win_cache); }

/* ... and a thread that ends without calling it does not keep them: a key whose destructor frees the thread's set */
static pthread_key_t g_win_cache_key;
static pthread_once_t g_win_cache_once = PTHREAD_ONCE_INIT;
static void win_cache_at_thread_exit(void *p)
{
    win_cache_free((struct win_cache *)p);
}
static void win_cache_make_key(void) { (void)pthread_key_create(&g_win_cache_key, win_cache_at_thread_exit); }
static void win_cache_arm(struct win_cache *c)
{
    (void)pthread_once(&g_win_cache_once, win_cache_make_key);
    (void)pthread_setspecific(g_win_cache_key, c);
}

static void windows_free(struct track_windows *w)
{
    if (!w)
        return;
    if (w->th_started) {
        pthread_mutex_lock(&w->mu);
        w->stop = 1;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
        pthread_join(w->th, NULL);
    }
    /* the buffers go to this thread's cache (whatever it held before is freed: the newer set fits the newer tracks) */
    struct win_cache *c = &t_win_cache;
    win_cache_free(c);
    c->valid = 1;
    win_cache_arm(c);
    c->device = w->opts.device;
    c->b = w->b;
    c->dev_bytes = w->dev_peak;
    for (int i = 0; i < WIN_SLOTS; i++) {
        c->slot[i] = w->slot[i];
        c->slot[i].frames = 0;
        rep_reset(&c->slot[i].rep);
    }
    free(w->rep.ng_blocks);
    free(w->whole);
    free(w->pack_tmp);
    free(w->spans);
    free(w->cw.p_spans);
    (void)hipFree(w->cw.d_zero);
    aob_close_all(&w->aobs);
    pthread_mutex_destroy(&w->mu);
    pthread_cond_destroy(&w->cv);
    free(w);
}

/* Does every substream of the sync unit at `off` of the stream [0, len) in d_stream open with a restart header?  (Reference:
 * decode_block src/mlp.c:748-753 -- two flags in front of a block, "parameters present" and "restart header present";
 * the unit's layout: 4 bytes of frame header, the 28-byte major sync with substream_count 128 bits in, src/mlp.c:621-632,
 * one directory word per substream and one more behind it when its top bit is set, src/mlp.c:463-468, 661-667.)
 * 1 = yes, 0 = no, -1 = the device read failed.  A window may begin at such a unit: the restart header sets every
 * parameter the lanes do not carry across a cut, the FIR history is carried (win_produce). */
static int win_unit_restarts(struct track_windows *w, uint64_t off, uint64_t len)
{
    uint8_t h[4 + 28 + 8 + 1];
    const uint64_t have = len - off < sizeof(h) ? len - off : sizeof(h);
    if (have < 4 + 28 + 2 + 1)
        return 0;
    if (hipMemcpy(h, w->b.d_stream + off, have, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (h[4] != 0xF8 || h[5] != 0x72 || h[6] != 0x6F || h[7] != 0xBB)
        return 0;
    const unsigned S = h[4 + 16] >> 4;
    if (S != 1 && S != 2)
        return 0;
    uint64_t p = 4 + 28, end0 = 0;
    for (unsigned s = 0; s < S; s++) {
        if (p + 2 > have)
            return 0;
        const unsigned e = ((unsigned)h[p] << 8) | h[p + 1];
        if (s == 0)
            end0 = (uint64_t)(e & 0xFFFu) * 2;
        p += (e & 0x8000u) ? 4 : 2;
    }
    if (p >= have || (h[p] & 0xC0) != 0xC0)
        return 0;
    if (S == 2) {
        uint8_t b = 0;
        if (off + p + end0 >= len)
            return 0;
        if (hipMemcpy(&b, w->b.d_stream + off + p + end0, 1, hipMemcpyDeviceToHost) != hipSuccess)
            return -1;
        if ((b & 0xC0) != 0xC0)
            return 0;
    }
    return 1;
}

/* the last segment of the index (a live one: a sync pattern inside another segment's frames is not a cut) -> its number
 * and byte offset; 0 when the stream has no segment start behind its first byte, -1 when a device call failed (that is
 * not "no cut": taken as one, the carried bytes would grow window after window).  restart_len != 0: the last one a
 * window can BEGIN at -- a major sync does not oblige the substreams to restart (the reference reads its parameters and
 * decodes on, src/mlp.c:449-460), and a lane that starts there would have no parameters; such a unit stays inside its
 * window, where the sequential pass reaches it with the state of the units before it.  restart_len = the stream's length. */
static int win_last_cut(struct track_windows *w, uint32_t n_seg, uint64_t restart_len, uint32_t *seg_out, uint64_t *off_out)
{
    for (uint32_t s = n_seg; s-- > 0;) {
        dvda_mlp_segment_info si;
        if (dvda_mlp_hip_segment_info(w->b.ctx, s, &si, NULL) != DVDA_HIP_OK)
            return -1;
        if (si.status & DVDA_ST_FALSE_SYNC)
            continue;
        if (restart_len && si.offset != 0) {
            const int r = win_unit_restarts(w, si.offset, restart_len);
            if (r < 0)
                return -1;
            if (!r)
                continue;
        }
        *seg_out = s;
        *off_out = si.offset;
        return si.offset != 0;
    }
    return 0;
}

/* ---- conceal mode across windows.  The rule is the batch tier's, stated for a track's whole stream (dvda_mlp_hip.h);
 * a window [0, cut) is decoded as a conceal-mode stream of its own, and what the batch tier cannot see is stitched here:
 * a window's TRAILING span, whole windows that kept nothing and the next window's LEADING span are ONE span, whose silence
 * -- the input-timing gap between the kept units on both sides, wrapped by the running mean of bytes per frame -- goes
 * out in front of the next kept window as silent windows of bounded size. */
#define SILENT_WINDOW_FRAMES 8192u

/* conceal_gap of csrc/mlp_conceal_run.h: g + 65536 w frames, w >= 0 bringing B bytes per frame closest to m (no mean: g) */
static uint64_t gap_frames(uint64_t B, uint32_t g, double m)
{
    if (!(m > 0.0))
        return g;
    double w0 = floor(((double)B / m - (double)g) / 65536.0);
    if (w0 < 0.0)
        w0 = 0.0;
    uint64_t best = 0;
    double bd = 0.0;
    for (int k = 0; k < 2; k++) {
        const uint64_t G = (uint64_t)g + 65536ull * ((uint64_t)w0 + (uint64_t)k);
        const double d = G ? fabs((double)B / (double)G - m) : INFINITY;
        if (k == 0 || d < bd) {
            best = G;
            bd = d;
        }
    }
    return best;
}

static int cw_span(struct track_windows *w, uint64_t first, uint64_t frames, uint64_t off, uint64_t end, uint32_t cause,
                   uint32_t flags)
{
    if (w->cw.p_n == w->cw.p_cap) {
        const unsigned cap = w->cw.p_cap ? 2 * w->cw.p_cap : 16;
        dvda_mlp_conceal_span *g = realloc(w->cw.p_spans, cap * sizeof(*g));
        if (!g)
            return 0;
        w->cw.p_spans = g;
        w->cw.p_cap = cap;
    }
    const dvda_mlp_conceal_span s = {first, frames, off, end, cause ? cause : DVDA_ST_NO_SYNC, flags};
    w->cw.p_spans[w->cw.p_n++] = s;
    w->p_status |= DVDA_ST_CONCEALED;
    return 1;
}

/* `bytes` of the stream in front of d_stream[0 + ...] hold nothing to keep: they join the pending span */
static void cw_drop(struct track_windows *w, uint64_t bytes, uint32_t cause)
{
    w->cw.B += bytes;
    w->cw.cause |= cause;
    w->cw.base += bytes;
}

/* the track ends: what is pending is its TRAILING span (LEADING too when nothing was ever kept) */
static int cw_finish(struct track_windows *w)
{
    if (w->cw.B == 0 && w->cw.have_edge)
        return 1;
    if (w->cw.base == 0)
        return 1;                                /* (an empty track) */
    return cw_span(w, w->cw.frames, 0, w->cw.pend_off, w->cw.base, w->cw.cause,
                   DVDA_CONCEAL_TRAILING | (w->cw.have_edge ? 0u : DVDA_CONCEAL_LEADING));
}

/* The window [0, cut) has been decoded in conceal mode: its spans and edges -> the track's spans, the silence in front of
 * it (*gap frames) and the history the next window starts with.  1 = ok. */
static int win_conceal_stitch(struct track_windows *w, uint64_t cut, const dvda_mlp_stream_info *info, int final, uint64_t *gap)
{
    struct track_bufs *b = &w->b;
    dvda_mlp_conceal_edges e;
    dvda_mlp_conceal_span *sp = NULL;
    uint32_t n = 0, lead = 0, trail = 0, all = 0;
    int ok = 0;
    *gap = 0;
    if (dvda_mlp_hip_conceal_edges(b->ctx, 0, &e, NULL) != DVDA_HIP_OK ||
        dvda_mlp_hip_conceal_spans(b->ctx, 0, NULL, 0, &n, NULL) != DVDA_HIP_OK ||
        (sp = malloc((n ? n : 1) * sizeof(*sp))) == NULL ||
        dvda_mlp_hip_conceal_spans(b->ctx, 0, sp, n, &n, NULL) != DVDA_HIP_OK)
        goto out;
    for (uint32_t i = 0; i < n; i++) {
        all |= sp[i].cause;
        if (sp[i].flags & DVDA_CONCEAL_LEADING)
            lead |= sp[i].cause;
        if (sp[i].flags & DVDA_CONCEAL_TRAILING)
            trail |= sp[i].cause;
    }
    const int kept = e.kept_end > e.kept_begin;
    if (!kept) {
        cw_drop(w, cut, all);
    } else {
        w->cw.B += e.kept_begin;
        w->cw.cause |= lead;
        if (w->cw.have_edge && w->cw.B > 0) {
            const uint64_t kb = w->cw.kept_bytes + e.kept_bytes, kf = w->cw.kept_frames + e.kept_frames;
            *gap = gap_frames(w->cw.B, (e.t_first - w->cw.t_end) & 0xFFFFu, kb && kf ? (double)kb / (double)kf : 0.0);
            if (!cw_span(w, w->cw.frames, *gap, w->cw.pend_off, w->cw.base + e.kept_begin, w->cw.cause, 0))
                goto out;
        } else if (!w->cw.have_edge && w->cw.base + e.kept_begin > 0) {
            if (!cw_span(w, 0, 0, 0, w->cw.base + e.kept_begin, w->cw.cause, DVDA_CONCEAL_LEADING))
                goto out;
        }
        for (uint32_t i = 0; i < n; i++)
            if (!(sp[i].flags & (DVDA_CONCEAL_LEADING | DVDA_CONCEAL_TRAILING)) &&
                !cw_span(w, w->cw.frames + *gap + sp[i].first_frame, sp[i].frames, w->cw.base + sp[i].byte_off,
                         w->cw.base + sp[i].byte_end, sp[i].cause, sp[i].flags))
                goto out;
        w->cw.frames += *gap + info->pcm_frames;
        w->cw.have_edge = 1;
        w->cw.t_end = e.t_end;
        w->cw.kept_bytes += e.kept_bytes;
        w->cw.kept_frames += e.kept_frames;
        w->cw.B = e.ends_kept ? 0 : cut - e.kept_end;
        w->cw.cause = e.ends_kept ? 0 : trail;
        w->cw.pend_off = w->cw.base + e.kept_end;
        w->cw.base += cut;
    }
    /* the next window: the history behind a range that ends kept; behind damage a fresh decoder -- an explicit zero
       history (with none at all a first segment that continues the history would be DVDA_ST_ENVELOPE) */
    if (!final) {
        if (kept && e.ends_kept)
            memcpy(w->fir, e.fir, sizeof(w->fir));
        else
            memset(w->fir, 0, sizeof(w->fir));
        w->have_fir = 1;
    }
    ok = 1;
out:
    free(sp);
    return ok;
}

/* the decoded window in b->d_pcm -> its reports and the pinned slot */
static int win_deliver(struct track_windows *w, struct win_slot *out, const dvda_mlp_stream_info *info, uint64_t stride)
{
    struct track_bufs *b = &w->b;
    if (!piece_reports(&w->rep, &out->rep, w->wav_bits != 0, b->d_pcm, layout_of(w->wav_bits), bits_of(info->group0_bps),
                       stride, info->pcm_frames, info->channels, w->rep_before))
        return 0;
    w->rep_before += info->pcm_frames;
    const size_t bytes = (size_t)info->pcm_frames * info->channels * (w->wav_bits ? (unsigned)w->wav_bits / 8 : 4);
    if (!slot_reserve(b, out, bytes) ||
        (bytes && hipMemcpy(out->host, b->d_pcm, bytes, hipMemcpyDeviceToHost) != hipSuccess))
        return 0;
    out->frames = info->pcm_frames;
    w->p_frames += info->pcm_frames;
    win_dev_sample(w);
    return 1;
}

/* one silent window of at most SILENT_WINDOW_FRAMES of the silence that is left: zeros on the device, reports and copy
   as for any other window */
static int win_silence(struct track_windows *w, struct win_slot *out)
{
    dvda_mlp_stream_info info = w->cw.held_info;
    const uint64_t n = w->cw.sil_left < SILENT_WINDOW_FRAMES ? w->cw.sil_left : SILENT_WINDOW_FRAMES;
    const size_t cap = (size_t)SILENT_WINDOW_FRAMES * info.channels * sizeof(int32_t) + 64;
    if (!w->cw.d_zero && !dev_alloc((void **)&w->cw.d_zero, cap))
        return 0;
    if (hipMemsetAsync(w->cw.d_zero, 0, cap, NULL) != hipSuccess)
        return 0;
    info.pcm_frames = n;
    int32_t *const keep = w->b.d_pcm;
    w->b.d_pcm = w->cw.d_zero;                   /* (win_deliver reads the set's PCM buffer) */
    const int ok = win_deliver(w, out, &info, SILENT_WINDOW_FRAMES);
    w->b.d_pcm = keep;
    w->cw.sil_left -= n;
    return ok;
}

/* stream bytes [from, from + keep) of d_stream wait on the host for the next window (conceal mode sizes the buffer with
   little to spare: what a reader holds under damage is measured against a clean track's) */
static int win_carry(struct track_windows *w, uint64_t from, uint64_t keep)
{
    struct track_bufs *b = &w->b;
    if (keep > b->carry_cap) {
        free(b->carry);
        b->host_now -= b->carry_cap;
        b->carry_cap = keep + (w->opts.conceal ? 0 : keep / 2) + 4096;
        b->carry = malloc(b->carry_cap);
        if (!b->carry) {
            b->carry_cap = 0;
            return 0;
        }
        bufs_host_add(b, b->carry_cap);
    }
    if (keep && hipMemcpy(b->carry, b->d_stream + from, keep, hipMemcpyDeviceToHost) != hipSuccess)
        return 0;
    w->carry_len = keep;
    return 1;
}

/* One window into `out`: 1 = out holds frames (possibly none), 0 = failure.  Leaves "this was the track's last window",
 * the window's status bits and its frame count in w->p_*: the caller publishes them (win_commit, under w->mu once a
 * consumer exists).  Runs in the opener's thread for the first window, in the producer thread afterwards. */
static int win_produce(struct track_windows *w, struct win_slot *out)
{
    struct track_bufs *b = &w->b;
    unsigned in_track, got = 0;
    int final;
    uint64_t total = 0, begin = 0, end = 0, stride = 0;
    out->frames = 0;
    out->stride = 0;
    rep_reset(&out->rep);
    const int conceal = w->opts.conceal;
    w->p_final = 0;
    /* ---- conceal mode: silence that is still owed, then the decoded window that waits behind it */
    if (w->cw.sil_left)
        return win_silence(w, out);
    if (w->cw.held) {
        w->cw.held = 0;
        if (!win_deliver(w, out, &w->cw.held_info, w->cw.held_stride))
            return 0;
        w->p_final = w->cw.held_final;
        return 1;
    }
    /* ---- sectors -> device -> MLP bytes, and where this window's new bytes begin and end: the end-of-track rule on
       the window that holds the track's last sector, with its look-ahead */
    for (unsigned extra = 8;; extra *= 4) {
        in_track = w->next <= w->last ? w->last - w->next + 1 : 0;
        final = in_track <= w->window;
        if (!final)
            in_track = w->window;
        unsigned want = in_track + (final ? extra : 0);
        if (w->next + want > w->aobs.total || w->next + want < w->next)
            want = w->aobs.total - w->next;
        if (!sectors_to_device(b, &w->aobs, w->next, want, 0, 0, NULL, &got, &total, NULL))
            return 0;
        if (!got && !final)
            return 0;                            /* the files end inside the track */
        const int rc = stream_bounds(b, !w->started, final, in_track, got, want, w->next + got >= w->aobs.total, total,
                                     &begin, &end);
        if (rc < 0)
            return 0;
        if (rc)
            break;
    }
    if (end < begin)
        end = begin;
    /* ---- the stream of this window: what was kept + the new bytes */
    uint64_t len = w->carry_len + (end - begin);
    if (!bufs_dev_room(b, (void **)&b->d_stream, &b->cap_stream, ((len + 15) & ~(uint64_t)15) + 64 + 16))
        return 0;
    if ((w->carry_len && hipMemcpy(b->d_stream, b->carry, w->carry_len, hipMemcpyHostToDevice) != hipSuccess) ||
        (end > begin && hipMemcpy(b->d_stream + w->carry_len, b->d_mlp + begin, end - begin, hipMemcpyDeviceToDevice) != hipSuccess))
        return 0;
    w->next += final ? got : in_track;
    w->started = 1;
    if (len == 0) {
        w->p_final = final;
        if (conceal && final && !cw_finish(w))
            return 0;
        return final;                        /* an empty track does not open */
    }
    uint32_t n_seg = 0, cut_seg = 0;
    uint64_t cut = len;
    int forced = 0;
    if (!index_stream(b, &w->opts, len, &n_seg))
        return 0;
    if (!final) {
        const int have_cut = win_last_cut(w, n_seg, len, &cut_seg, &cut);
        if (have_cut < 0)
            return 0;
        if (!have_cut) {
            /* no segment starts inside this window: all of it waits for the next one */
            cut = 0;
            /* conceal mode, bounded memory under damage: more than a window's payload waiting and still no cut --
               [0, len) is decoded as it is; if it ends kept (one long clean segment) it waits as ever, else what is kept
               goes out and the rest joins the pending span: nothing is carried.  (What waits is then never more than a
               window's payload: what the reader holds stays within one window of a clean track's.) */
            forced = conceal && len > (uint64_t)w->window * 2021u;
        }
        /* what follows the cut is kept (host copy: the device buffers are the next window's); a window that is decoded
           whole keeps its bytes only if it turns out to end kept (below) */
        if (forced)
            w->carry_len = 0;
        else if (!win_carry(w, cut, len - cut))
            return 0;
        if (cut == 0 && !forced)
            return 1;                        /* nothing to decode yet (out->frames == 0) */
        if (forced)
            cut = len;                       /* (the index of [0, len) is the one just made) */
        else if (!index_stream(b, &w->opts, cut, &n_seg))     /* the index of what is decoded now: whole segments */
            return 0;
    } else {
        w->carry_len = 0;
    }
    if (conceal && n_seg == 0 && (final || forced)) {
        /* not one major sync in these bytes: nothing to decode, nothing to keep */
        cw_drop(w, cut, DVDA_ST_NO_SYNC);
        w->carry_len = 0;
        memset(w->fir, 0, sizeof(w->fir));
        w->have_fir = 1;
        w->p_final = final;
        return !final || cw_finish(w);
    }
    /* ---- decode [0, cut) from the history the window before left (the payload or int32 frames: the bit depth is in
       the index's stream record, known before anything is decoded) */
    dvda_mlp_stream_info info;
    if (!decode_stream(b, cut, w->have_fir ? w->fir : NULL, &w->wav_bits, &info, &stride, &w->opts))
        return 0;
    w->p_status |= info.status;
    if (info.status & ~(uint32_t)(DVDA_ST_BENIGN | (conceal ? DVDA_ST_CONCEALED : 0u)))
        return 0;                            /* the reference assert()s on such a stream */
    if (!w->info.channels)
        w->info = info;
    if (conceal) {
        /* ---- the window's spans and edges join the track's; the history comes from the edges */
        uint64_t gap = 0;
        if (forced) {
            dvda_mlp_conceal_edges e;
            if (dvda_mlp_hip_conceal_edges(b->ctx, 0, &e, NULL) != DVDA_HIP_OK)
                return 0;
            if (e.ends_kept)
                return win_carry(w, 0, len); /* a long clean segment: it waits for its end as ever */
        }
        if (!win_conceal_stitch(w, cut, &info, final, &gap))
            return 0;
        if (final && !cw_finish(w))
            return 0;
        if (gap) {
            w->cw.sil_left = gap;
            w->cw.held = 1;
            w->cw.held_final = final;
            w->cw.held_info = info;
            w->cw.held_stride = stride;
            return win_silence(w, out);
        }
        if (!win_deliver(w, out, &info, stride))
            return 0;
        w->p_final = final;
        return 1;
    }
    /* ---- the history at the cut, for the next window */
    if (!final) {
        uint32_t last_seg = 0;
        uint64_t dummy = 0;
        if (win_last_cut(w, n_seg, 0, &last_seg, &dummy) < 0)
            return 0;
        if (dvda_mlp_hip_segment_fir(b->ctx, last_seg, w->fir, NULL) != DVDA_HIP_OK)
            return 0;
        w->have_fir = 1;
    }
    /* ---- the window's reports, from the device */
    if (!piece_reports(&w->rep, &out->rep, w->wav_bits != 0, b->d_pcm, layout_of(w->wav_bits), bits_of(info.group0_bps),
                       stride, info.pcm_frames, info.channels, w->rep_before))
        return 0;
    w->rep_before += info.pcm_frames;
    /* ---- PCM (or payload) to the host buffer */
    const size_t bytes = (size_t)info.pcm_frames * info.channels * (w->wav_bits ? (unsigned)w->wav_bits / 8 : 4);
    if (!slot_reserve(b, out, bytes) ||
        (bytes && hipMemcpy(out->host, b->d_pcm, bytes, hipMemcpyDeviceToHost) != hipSuccess))
        return 0;
    out->frames = info.pcm_frames;
    w->p_frames += info.pcm_frames;
    win_dev_sample(w);
    w->p_final = final;
    return 1;
}

/* One window of a raw-PCM track into `out` (reference: src/dvd-audio.c:1017-1083 decode_pcm_audio packet by packet,
 * src/pcm.c:99-193): the next run of sectors -> device -> k_pcm_scan / k_pcm_unswizzle_t -> the pinned slot, planar int32
 * or the packed payload.  A track that spills over its sector range reads on.  1 = ok (out->frames may be 0),
 * 0 = failure. */
static int win_produce_pcm(struct track_windows *w, struct win_slot *out)
{
    struct track_bufs *b = &w->b;
    const unsigned bits = w->pcm_bits, ch = w->pcm_channels;
    unsigned want = w->window, got = 0;
    uint64_t total = 0, stride = 0;
    int final = 0;
    out->frames = 0;
    out->stride = 0;
    rep_reset(&out->rep);
    if (w->next + want > w->aobs.total || w->next + want < w->next)
        want = w->next < w->aobs.total ? w->aobs.total - w->next : 0;
    if (!sectors_to_device(b, &w->aobs, w->next, want, bits, ch, NULL, &got, &total, &stride))
        return 0;
    if (!got) {
        w->p_final = 1;
        return w->started;                       /* the files end: what was delivered stands */
    }
    const uint64_t deliver = pcm_deliver(b->h_base, got, total, w->pcm_done, w->pcm_want, &final);
    w->next += got;
    w->started = 1;
    if (!final && (got < want || w->next >= w->aobs.total))
        final = 1;                               /* the files end inside the track */
    /* (the planes as the un-swizzle left them: before packing and copy; a reader that reduces the word length has the
       reports of its int32 PCM, as an MLP reader in its place has) */
    if (!piece_reports(&w->rep, &out->rep, w->wav_bits != 0 && !rq_applies(&w->opts, bits), b->d_pcm, DVDA_PCM_PLANAR, bits,
                       stride, deliver, ch, w->rep_before))
        return 0;
    w->rep_before += deliver;
    if (deliver && w->wav_bits) {
        /* (at the depth the reader hands out: the track's, or what it was reduced to just now) */
        const size_t bytes = (size_t)deliver * ch * (w->pcm_out_bits / 8);
        if (!bufs_dev_room(b, (void **)&b->d_stream, &b->cap_stream, bytes + 64) ||
            dvda_mlp_hip_pack_wav(b->d_pcm, stride, ch, deliver, w->pcm_out_bits, b->d_stream, NULL) != DVDA_HIP_OK ||
            !slot_reserve(b, out, bytes) ||
            hipMemcpy(out->host, b->d_stream, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return 0;
    } else if (deliver) {
        /* the window's frames of every channel, the planes packed to `deliver` frames each */
        if (!slot_reserve(b, out, (size_t)deliver * ch * sizeof(int32_t)) ||
            hipMemcpy2D(out->host, (size_t)deliver * sizeof(int32_t), b->d_pcm, (size_t)stride * sizeof(int32_t),
                        (size_t)deliver * sizeof(int32_t), ch, hipMemcpyDeviceToHost) != hipSuccess)
            return 0;
        out->stride = deliver;
    }
    out->frames = deliver;
    w->pcm_done += deliver;
    w->p_frames += deliver;
    w->p_final = final;
    win_dev_sample(w);
    return 1;
}

/* publishes what the last produce() left (the caller holds w->mu, or no consumer exists yet) */
static void win_commit(struct track_windows *w)
{
    w->status |= w->p_status;
    w->frames_total += w->p_frames;
    w->p_frames = 0;
    if (w->cw.p_n) {
        if (w->n_spans + w->cw.p_n > w->cap_spans) {
            const unsigned cap = 2 * (w->n_spans + w->cw.p_n);
            dvda_mlp_conceal_span *g = realloc(w->spans, cap * sizeof(*g));
            if (g) {
                w->spans = g;
                w->cap_spans = cap;
            } else {
                w->failed = 1;
            }
        }
        if (w->n_spans + w->cw.p_n <= w->cap_spans) {
            memcpy(w->spans + w->n_spans, w->cw.p_spans, w->cw.p_n * sizeof(*w->spans));
            w->n_spans += w->cw.p_n;
        }
        w->cw.p_n = 0;
    }
    if (w->p_final)
        w->finished = 1;
}

static void *win_thread(void *arg)
{
    struct track_windows *w = arg;
    if (hipSetDevice(w->opts.device) != hipSuccess) {
        pthread_mutex_lock(&w->mu);
        w->failed = 1;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
        return NULL;
    }
    for (;;) {
        pthread_mutex_lock(&w->mu);
        while (!w->stop && w->count == WIN_SLOTS)
            pthread_cond_wait(&w->cv, &w->mu);
        if (w->stop || w->finished || w->failed) {
            pthread_mutex_unlock(&w->mu);
            break;
        }
        struct win_slot *out = &w->slot[w->head];
        pthread_mutex_unlock(&w->mu);
        const int ok = w->produce(w, out);
        pthread_mutex_lock(&w->mu);
        win_commit(w);                          /* status, frames and "finished" together with the window itself */
        if (!ok)
            w->failed = 1;
        else if (out->frames) {
            w->head = (w->head + 1) % WIN_SLOTS;
            w->count++;
        }
        pthread_cond_broadcast(&w->cv);
        const int done = w->finished || w->failed;
        pthread_mutex_unlock(&w->mu);
        if (done)
            break;
    }
    return NULL;
}

/* the window the consumer reads from: waits for the producer; NULL at the end of the track (or on failure) */
static struct win_slot *win_current(struct track_windows *w)
{
    struct win_slot *s = NULL;
    pthread_mutex_lock(&w->mu);
    while (w->count == 0 && !w->finished && !w->failed)
        pthread_cond_wait(&w->cv, &w->mu);
    if (w->count)
        s = &w->slot[w->tail];
    pthread_mutex_unlock(&w->mu);
    return s;
}
static void win_release(struct track_windows *w)
{
    pthread_mutex_lock(&w->mu);
    reports_join(&w->rep, &w->slot[w->tail].rep);
    w->tail = (w->tail + 1) % WIN_SLOTS;
    w->count--;
    w->served_in_slot = 0;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
}

/* A windowed reader of track k, nothing read yet: its records, the buffers the thread's last windowed reader left (same
 * device: its context and buffers serve this track too), the memory baseline and its own open files.  NULL = failure. */
static DVDA_Track_Reader *windows_new(const DVDA_Track *k, const struct reader_opts *o, dvda_codec_t codec,
                                      int (*produce)(struct track_windows *, struct win_slot *))
{
    struct track_windows *w = calloc(1, sizeof(*w));
    DVDA_Track_Reader *r = calloc(1, sizeof(*r));
    struct win_cache *c = &t_win_cache;
    size_t tot = 0;
    if (!w || !r) {
        free(w);
        free(r);
        return NULL;
    }
    pthread_mutex_init(&w->mu, NULL);
    pthread_cond_init(&w->cv, NULL);
    r->win = w;
    r->codec = codec;
    r->interleaved = 1;
    w->produce = produce;
    w->opts = *o;
    rep_want(&w->rep, o);
    w->next = k->s.first;
    w->last = k->s.last >= k->s.first ? k->s.last : k->s.first;
    w->window = window_sectors();
    if (c->valid && c->device != o->device)
        win_cache_free(c);
    if (c->valid) {
        w->b = c->b;
        w->b.host_peak = w->b.host_now;
        for (int i = 0; i < WIN_SLOTS; i++)
            w->slot[i] = c->slot[i];
        w->dev_base = w->dev_peak = c->dev_bytes;
        memset(c, 0, sizeof(*c));
    }
    w->b.pinned = 1;
    (void)hipMemGetInfo(&w->dev_free0, &tot);
    aob_open_all(&w->aobs, k->dir, k->titleset);
    if (w->aobs.n == 0) {
        reader_free(r);
        return NULL;
    }
    return r;
}

/* The first window in the opener's thread -- what the stream is is known when the reader is handed out -- and the
 * producer thread for the rest.  0 = failure. */
static int windows_start(struct track_windows *w)
{
    struct win_slot *out = &w->slot[0];
    for (;;) {
        const int ok = w->produce(w, out);
        win_commit(w);                          /* (no consumer yet: no lock needed) */
        if (!ok)
            return 0;
        if (out->frames || w->finished)
            break;
    }
    if (out->frames) {
        w->head = 1 % WIN_SLOTS;
        w->count = 1;
    }
    if (!w->finished) {
        if (pthread_create(&w->th, NULL, win_thread, w) != 0)
            return 0;
        w->th_started = 1;
    }
    return 1;
}

static DVDA_Track_Reader *open_mlp_windowed(const DVDA_Track *k, const struct reader_opts *o)
{
    DVDA_Track_Reader *r = windows_new(k, o, DVDA_MLP, win_produce);
    if (!r)
        return NULL;
    struct track_windows *w = r->win;
    w->wav_bits = o->wav_output ? -1 : 0;       /* (win_produce decides it from the first window's index) */
    /* (w->info is written once, by the first window that decodes: the producer thread only reads it) */
    /* (a track that would be decimated is not read in windows: a later change; dvda_pcm_decim_piece carries what it needs.
       An MLP stream names its rate in its first major sync only, so the refusal comes after windows_start has decoded
       the first window and started the producer thread -- work thrown away, on a path that ends in NULL either way; a
       raw-PCM track's packet header has the rate, and open_pcm_windowed refuses before it starts anything) */
    if (!windows_start(w) || !w->info.channels || !mlp_info_to_reader(r, &w->info, o->present) ||
        dc_applies(o, w->info.group0_rate) || rs_applies(o, w->info.group0_rate) || mx_applies(o, r->channels)) {
        reader_free(r);
        return NULL;
    }
    if (rq_applies(o, bits_of(w->info.group0_bps))) {
        r->src_bits = bits_of(w->info.group0_bps);
        r->bps_code[0] = code_of_bits(o->rq_bits);
    }
    return r;
}

/* ------------------------------------------------------------------ PCM track */
static uint64_t pcm_track_frames(const DVDA_Track *k, unsigned rate)
{
    return (uint64_t)lround((double)k->s.pts_length * (double)rate / DVDA_HIP_PTS_PER_SECOND);
}

static DVDA_Track_Reader *open_pcm(struct aob_set *aobs, const DVDA_Track *k, const uint8_t *params,
                                   const struct reader_opts *o)
{
    DVDA_Track_Reader *r = calloc(1, sizeof(*r));
    struct track_bufs b;
    unsigned bits = 0, rate = 0, got = 0;
    uint64_t total = 0, stride = 0, deliver = 0;
    memset(&b, 0, sizeof(b));
    if (!r)
        return NULL;
    r->codec = DVDA_PCM;
    if (!pcm_params_to_reader(r, params, &bits, &rate))
        goto fail;
    const uint64_t want_frames = pcm_track_frames(k, rate);
    const unsigned first = k->s.first;
    for (unsigned count = k->s.last >= first ? k->s.last - first + 1 : 1;; count *= 2) {
        int covered = 0;
        if (first + count > aobs->total || first + count < first)
            count = aobs->total - first;
        bufs_free(&b);
        if (!sectors_to_device(&b, aobs, first, count, bits, r->channels, NULL, &got, &total, &stride) || !got)
            goto fail;
        deliver = pcm_deliver(b.h_base, got, total, 0, want_frames, &covered);
        if (covered || got != count || first + got >= aobs->total)
            break;                               /* (else the track spills over its sector range) */
    }
    r->frames = deliver;
    r->d_pcm = b.d_pcm;
    b.d_pcm = NULL;
    if (!track_passes(r, o, &r->d_pcm, DVDA_PCM_PLANAR, 0, stride))
        goto fail;
    goto done;
fail:
    reader_free(r);
    r = NULL;
done:
    bufs_free(&b);
    return r;
}

/* A raw-PCM track of more sectors than a window: read, un-swizzled and handed out window by window (round 6; the
 * reference streams a track of any length packet by packet, src/dvd-audio.c:752-795, 1017-1083).  The first window in
 * the opener's thread, the rest by the producer thread into the two pinned slots: what the reader holds is bounded by
 * the window, not by the track. */
static DVDA_Track_Reader *open_pcm_windowed(const DVDA_Track *k, const uint8_t *params, const struct reader_opts *o)
{
    DVDA_Track_Reader *r = windows_new(k, o, DVDA_PCM, win_produce_pcm);
    unsigned bits = 0, rate = 0;
    if (!r)
        return NULL;
    struct track_windows *w = r->win;
    if (!pcm_params_to_reader(r, params, &bits, &rate) || dc_applies(o, r->rate_code[0]) || rs_applies(o, r->rate_code[0]) ||
        mx_applies(o, r->channels)) {
        reader_free(r);
        return NULL;
    }
    w->pcm_bits = bits;
    w->pcm_out_bits = rq_applies(o, bits) ? o->rq_bits : bits;
    w->pcm_channels = r->channels;
    w->pcm_want = pcm_track_frames(k, rate);
    w->wav_bits = o->wav_output && w->pcm_out_bits != 20 ? (int)w->pcm_out_bits : 0;
    r->src_bits = bits;
    r->bps_code[0] = code_of_bits(w->pcm_out_bits);
    if (!windows_start(w)) {
        reader_free(r);
        return NULL;
    }
    return r;
}

/* ------------------------------------------------------------------ track reader */
static DVDA_Track_Reader *open_reader(const DVDA_Track *k, const struct reader_opts *o)
{
    struct aob_set aobs;
    DVDA_Track_Reader *r = NULL;
    uint8_t sec[SECTOR];
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= o->device) {
        fprintf(stderr, "libdvd_audio_hip: no HIP device %d (the decode path is GPU-only)\n", o->device);
        return NULL;
    }
    if (hipSetDevice(o->device) != hipSuccess)
        return NULL;
    /* the word-length reduction: a depth and a mode it has; not together with conceal mode (the stitch between two
       windows rewrites frames that were handed over, and reduced, already) */
    if (o->rq_bits && ((o->rq_bits != 16 && o->rq_bits != 20 && o->rq_bits != 24) || o->rq_mode > DVDA_RQ_TPDF || o->conceal))
        return NULL;
    /* the decimation: a ratio it has; not together with conceal mode */
    if (o->dc_ratio && (!dc_shift(o) || o->conceal))
        return NULL;
    /* the resampler: the one rate it makes; not together with conceal mode or the decimation */
    if (o->rs_rate && (o->rs_rate != 44100 || o->conceal || o->dc_ratio))
        return NULL;
    /* the channel mix: one or two channels, flags it has; not together with conceal mode */
    if (o->mx_ch && (o->mx_ch > 2 || (o->mx_flags & ~(DVDA_MIX_UNITY | DVDA_MIX_LFE)) || o->conceal))
        return NULL;
    aob_open_all(&aobs, k->dir, k->titleset);
    if (aobs.n == 0 || k->s.first >= aobs.total)
        goto out;
    /* a long track is read and decoded window by window (bounded memory); a short one as one batch */
    const unsigned in_track = k->s.last >= k->s.first ? k->s.last - k->s.first + 1 : 1;
    const int windowed = in_track > window_sectors();
    /* the first audio packet at or after the track's first sector names the codec */
    for (unsigned s = k->s.first; s < aobs.total; s++) {
        unsigned codec = 0, pad2 = 0, body_len = 0;
        const uint8_t *body = NULL;
        if (aob_read(&aobs, s, 1, sec) != 1)
            break;
        const int rc = first_audio_packet(sec, &codec, &pad2, &body, &body_len);
        if (rc < 0 && o->conceal && s < k->s.last)
            continue;                            /* conceal mode: a malformed sector inside the track is not the end of it */
        if (rc < 0)
            break;
        if (rc == 0)
            continue;
        if (codec == CODEC_MLP)
            r = windowed ? open_mlp_windowed(k, o) : open_mlp(&aobs, k, o);
        else if (codec == CODEC_PCM && body_len >= 9 && pad2 >= 9)
            r = windowed ? open_pcm_windowed(k, body, o) : open_pcm(&aobs, k, body, o);
        break;
    }
    if (r)
        r->conceal = o->conceal;                /* (a raw-PCM track has nothing to conceal: no spans) */
out:
    aob_close_all(&aobs);
    return r;
}

/* the calling thread's options, as they are now */
DVDA_Track_Reader *dvda_open_track_reader(const DVDA_Track *k)
{
    const struct reader_opts o = opts_now();
    return open_reader(k, &o);
}

/* the options of THIS reader: the calling thread's defaults stay as they are, whatever happens */
DVDA_Track_Reader *dvda_hip_open_track_reader_with(const DVDA_Track *k, int device, int wav_output, int presentation)
{
    struct reader_opts o = opts_now();
    o.device = device;
    o.wav_output = wav_output != 0;
    o.present = presentation == 1;
    return open_reader(k, &o);
}

/* ... and conceal mode named too (< 0: as the thread, or the environment, has it) */
DVDA_Track_Reader *dvda_hip_open_track_reader_concealing(const DVDA_Track *k, int device, int wav_output, int presentation,
                                                         int conceal)
{
    struct reader_opts o = opts_now();
    o.device = device;
    o.wav_output = wav_output != 0;
    o.present = presentation == 1;
    if (conceal >= 0)
        o.conceal = conceal != 0;
    return open_reader(k, &o);
}

DVDA_Track_Reader *dvda_hip_open_track_reader_on(const DVDA_Track *k, int device, int wav_output)
{
    return dvda_hip_open_track_reader_with(k, device, wav_output, t_opts.present);
}

int dvda_hip_reader_wav_only(const DVDA_Track_Reader *r) { return r && (r->d_wav != NULL || (r->win && r->win->wav_bits)); }

void dvda_close_track_reader(DVDA_Track_Reader *r) { reader_free(r); }

dvda_codec_t dvda_codec(const DVDA_Track_Reader *r) { return r->codec; }
unsigned dvda_bits_per_sample(const DVDA_Track_Reader *r) { return bits_of(r->bps_code[0]); }
unsigned dvda_hip_reader_source_bits(const DVDA_Track_Reader *r) { return r->src_bits ? r->src_bits : bits_of(r->bps_code[0]); }
unsigned dvda_sample_rate(const DVDA_Track_Reader *r) { return rate_of(r->rate_code[0]); }
/* (the two accessors of the decimation take a NULL reader alike: no state, no rate) */
unsigned dvda_hip_reader_source_rate(const DVDA_Track_Reader *r)
{
    if (!r)
        return 0;
    return r->src_rate ? r->src_rate : rate_of(r->rate_code[0]);
}
int dvda_hip_reader_decimated(const DVDA_Track_Reader *r, dvda_pcm_decim_report *out)
{
    if (!r || !r->dc_done)
        return 0;
    if (out)
        *out = r->dc_rep;
    return 1;
}
int dvda_hip_reader_resampled(const DVDA_Track_Reader *r, dvda_pcm_decim_report *out)
{
    if (!r || !r->rs_done)
        return 0;
    if (out)
        *out = r->rs_rep;
    return 1;
}
unsigned dvda_channel_count(const DVDA_Track_Reader *r) { return r->src_channels ? r->channels : channels_of(r->assignment); }
unsigned dvda_hip_reader_source_channels(const DVDA_Track_Reader *r)
{
    if (!r)
        return 0;
    return r->src_channels ? r->src_channels : r->channels;
}
int dvda_hip_reader_downmixed(const DVDA_Track_Reader *r, dvda_pcm_mix_report *out)
{
    if (!r || !r->src_channels)
        return 0;
    if (out)
        *out = r->mx_rep;
    return 1;
}
unsigned dvda_hip_reader_status(const DVDA_Track_Reader *r)
{
    if (!r->win)
        return r->status;
    pthread_mutex_lock(&r->win->mu);
    const unsigned st = r->win->status;
    pthread_mutex_unlock(&r->win->mu);
    return st;
}
/* (a track read in windows knows its length when its last window has been decoded: until then, the frames so far) */
unsigned long long dvda_hip_reader_total_frames(const DVDA_Track_Reader *r)
{
    if (!r->win)
        return r->frames;
    pthread_mutex_lock(&r->win->mu);
    const unsigned long long n = r->win->frames_total;
    pthread_mutex_unlock(&r->win->mu);
    return n;
}
int dvda_hip_reader_windowed(const DVDA_Track_Reader *r) { return r && r->win != NULL; }
int dvda_hip_reader_failed(const DVDA_Track_Reader *r)
{
    int f = 0;
    if (r && r->win) {
        pthread_mutex_lock(&r->win->mu);
        f = r->win->failed;
        pthread_mutex_unlock(&r->win->mu);
    }
    return f;
}
/* the reader's reports as they stand: 1 = the track's, 0 = of the windows handed out so far, -1 = a failed reader */
static int reader_reports(const DVDA_Track_Reader *r, struct pcm_reports *out)
{
    if (!r->win) {
        *out = r->rep;
        return 1;
    }
    struct track_windows *w = r->win;
    pthread_mutex_lock(&w->mu);
    *out = w->rep;
    /* final: the producer is done and every window has been handed out */
    const int rc = w->failed ? -1 : (w->finished && w->count == 0) ? 1 : 0;
    pthread_mutex_unlock(&w->mu);
    return rc;
}
int dvda_hip_reader_crc32(const DVDA_Track_Reader *r, unsigned *crc, unsigned long long *bytes)
{
    struct pcm_reports rep;
    const int rc = r ? reader_reports(r, &rep) : -1;
    if (rc < 0 || rep.dg <= 0)
        return -1;
    if (crc)
        *crc = rep.crc;
    if (bytes)
        *bytes = rep.bytes;
    return rc;
}
int dvda_hip_reader_levels(const DVDA_Track_Reader *r, dvda_pcm_levels *out)
{
    struct pcm_reports rep;
    const int rc = r ? reader_reports(r, &rep) : -1;
    if (rc < 0 || rep.lv <= 0)
        return -1;
    if (out)
        *out = rep.levels;
    return rc;
}
int dvda_hip_reader_requantized(const DVDA_Track_Reader *r, dvda_pcm_requant_report *out)
{
    struct pcm_reports rep;
    const int rc = r ? reader_reports(r, &rep) : -1;
    if (rc < 0 || rep.rq <= 0)
        return -1;
    if (out)
        *out = rep.rq_rep;
    return rc;
}
int dvda_hip_reader_energy(const DVDA_Track_Reader *r, dvda_pcm_energy_block *blocks, unsigned long long cap,
                           unsigned long long *n)
{
    if (!r)
        return -1;
    /* (the blocks are copied under the lock: a window handed out meanwhile moves the track's array) */
    struct track_windows *w = r->win;
    int rc = 1;
    if (w)
        pthread_mutex_lock(&w->mu);
    const struct pcm_reports *rep = w ? &w->rep : &r->rep;
    if (w)
        rc = w->failed ? -1 : (w->finished && w->count == 0) ? 1 : 0;
    if (rep->ng <= 0)
        rc = -1;
    if (rc >= 0) {
        if (n)
            *n = rep->ng_n;
        for (uint64_t j = 0; blocks && j < cap && j < rep->ng_n; j++)
            blocks[j] = rep->ng_blocks[j];
    }
    if (w)
        pthread_mutex_unlock(&w->mu);
    return rc;
}
/* what was concealed of the track: 1 = final, 0 = not yet (a windowed reader that still produces), -1 = opened without
 * conceal mode */
int dvda_hip_reader_concealed(const DVDA_Track_Reader *r, struct dvda_mlp_conceal_span *spans, unsigned cap, unsigned *n)
{
    if (!r || !r->conceal)
        return -1;
    if (r->win) {
        /* a windowed reader: the spans of the windows produced so far; final once the last one has been */
        struct track_windows *w = r->win;
        pthread_mutex_lock(&w->mu);
        if (n)
            *n = w->n_spans;
        for (unsigned i = 0; spans && i < cap && i < w->n_spans; i++)
            spans[i] = w->spans[i];
        const int rc = w->failed ? -1 : w->finished ? 1 : 0;
        pthread_mutex_unlock(&w->mu);
        return rc;
    }
    if (n)
        *n = r->n_spans;
    for (unsigned i = 0; spans && i < cap && i < r->n_spans; i++)
        spans[i] = r->spans[i];
    return 1;
}
int dvda_hip_reader_memory(const DVDA_Track_Reader *r, unsigned long long *host_peak, unsigned long long *device_peak)
{
    if (!r || !r->win)
        return 0;
    if (host_peak)
        *host_peak = r->win->b.host_peak;
    if (device_peak)
        *device_peak = r->win->dev_peak;
    return 1;
}

unsigned dvda_riff_wave_channel_mask(const DVDA_Track_Reader *r)
{
    /* speaker bits per channel assignment (src/dvd-audio.c:693-755): the table the default mix matrices are made from */
    if (r->src_channels)
        return r->channels == 1 ? 0x4u : 0x3u;      /* the mix: FC, or FL | FR */
    return dvda_pcm_hip_speaker_mask(r->assignment);
}

unsigned dvda_read(DVDA_Track_Reader *r, unsigned pcm_frames, int buffer[])
{
    if (r->win) {
        /* a track read in windows: frames out of the window in hand, the next one when it is used up */
        struct track_windows *w = r->win;
        unsigned done = 0;
        if (w->wav_bits)
            return 0;           /* payload only (dvda_hip_reader_wav_next) */
        while (done < pcm_frames) {
            struct win_slot *s = win_current(w);
            if (!s)
                break;
            const uint64_t left = s->frames - w->served_in_slot;
            const unsigned n = left < pcm_frames - done ? (unsigned)left : pcm_frames - done;
            if (s->stride) {
                /* a raw-PCM window: planes of `stride` frames, interleaved here (src/dvd-audio.c:781-792) */
                for (unsigned c = 0; c < r->channels; c++) {
                    const int32_t *src = (const int32_t *)s->host + (size_t)c * s->stride + w->served_in_slot;
                    int *dst = buffer + (size_t)done * r->channels + c;
                    for (unsigned i = 0; i < n; i++)
                        dst[(size_t)i * r->channels] = src[i];
                }
            } else
            memcpy(buffer + (size_t)done * r->channels,
                   (const int32_t *)s->host + (size_t)w->served_in_slot * r->channels, (size_t)n * r->channels * sizeof(int32_t));
            w->served_in_slot += n;
            done += n;
            if (w->served_in_slot == s->frames)
                win_release(w);
        }
        r->served += done;
        return done;
    }
    if (r->d_wav)
        return 0;               /* opened under dvda_hip_set_wav_output(1): the track exists as WAV payload only */
    if (!r->pcm) {
        /* PCM of the whole track, fetched once */
        const size_t bytes = r->stride * r->channels * sizeof(int32_t);
        r->pcm = malloc(bytes ? bytes : 1);
        if (!r->pcm || hipMemcpy(r->pcm, r->d_pcm, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            free(r->pcm);
            r->pcm = NULL;
            return 0;
        }
    }
    const uint64_t left = r->frames - r->served;
    const unsigned n = left < pcm_frames ? (unsigned)left : pcm_frames;
    if (r->interleaved) {
        memcpy(buffer, r->pcm + (size_t)r->served * r->channels, (size_t)n * r->channels * sizeof(int32_t));
    } else {
        for (unsigned c = 0; c < r->channels; c++) {
            const int32_t *src = r->pcm + (size_t)c * r->stride + r->served;
            for (unsigned i = 0; i < n; i++)
                buffer[(size_t)i * r->channels + c] = src[i];
        }
    }
    r->served += n;
    return n;
}

/* The payload window by window: *payload = the next piece of the track's WAV data bytes (valid until the next call on
 * this reader), returns its size, 0 at the end of the track.  On a reader that is not windowed: the whole payload, once.
 * An int32 windowed reader (no wav output) is packed on the host, write_signed per value (src/bitstream.c:2846-2857). */
unsigned long long dvda_hip_reader_wav_next(DVDA_Track_Reader *r, const unsigned char **payload)
{
    *payload = NULL;
    if (!r->win)
        return r->served == 0 ? dvda_hip_reader_wav_payload(r, payload) : 0;
    struct track_windows *w = r->win;
    const unsigned bits = bits_of(r->bps_code[0]);
    if (bits != 16 && bits != 24)
        return 0;
    if (w->served_in_slot)                       /* the piece handed out by the call before: done with */
        win_release(w);
    struct win_slot *s = win_current(w);
    if (!s)
        return 0;
    const size_t nb = bits / 8;
    if (!w->wav_bits && s->stride) {
        /* a planar int32 window (raw PCM read without the payload option): packed into a buffer of its own */
        const size_t bytes = (size_t)s->frames * r->channels * nb;
        if (bytes > w->pack_cap) {
            free(w->pack_tmp);
            w->pack_cap = bytes + bytes / 4;
            w->pack_tmp = malloc(w->pack_cap);
            if (!w->pack_tmp) {
                w->pack_cap = 0;
                return 0;
            }
        }
        for (uint64_t i = 0; i < s->frames; i++)
            for (unsigned c = 0; c < r->channels; c++)
                pack_value(w->pack_tmp + (i * r->channels + c) * nb, ((const int32_t *)s->host)[(size_t)c * s->stride + i], bits);
        w->served_in_slot = s->frames;
        r->served += s->frames;
        *payload = w->pack_tmp;
        return (unsigned long long)bytes;
    }
    if (!w->wav_bits) {
        /* int32 frames -> payload, in place (the packed form is shorter) */
        const int32_t *src = (const int32_t *)s->host;
        uint8_t *dst = s->host;
        const uint64_t n = s->frames * r->channels;
        for (uint64_t i = 0; i < n; i++)
            pack_value(dst + i * nb, src[i], bits);
    }
    w->served_in_slot = s->frames;               /* released by the next call */
    r->served += s->frames;
    *payload = s->host;
    return (unsigned long long)s->frames * r->channels * nb;
}

unsigned long long dvda_hip_reader_wav_payload(DVDA_Track_Reader *r, const unsigned char **payload)
{
    if (r->win) {
        /* the whole payload of a windowed reader, for callers of the one-piece interface: every window appended (this
           is the one call on such a reader whose memory grows with the track) */
        struct track_windows *w = r->win;
        size_t have = 0, cap = 0;
        const unsigned char *piece = NULL;
        unsigned long long n;
        *payload = NULL;
        while ((n = dvda_hip_reader_wav_next(r, &piece)) != 0) {
            if (have + n > cap) {
                cap = (have + n) * 2;
                uint8_t *g = realloc(w->whole, cap);
                if (!g)
                    return 0;
                w->whole = g;
            }
            memcpy(w->whole + have, piece, n);
            have += n;
        }
        *payload = w->whole;
        return have;
    }
    const unsigned bits = bits_of(r->bps_code[0]);
    const uint64_t left = r->frames - r->served;
    const uint64_t bytes = left * r->channels * (bits / 8);
    uint8_t *d_out = NULL;
    *payload = NULL;
    if ((bits != 16 && bits != 24) || left == 0)
        return 0;
    if (r->d_wav) {
        /* the decode wrote the payload: one copy to the host */
        double t_mark = now_ms();
        free(r->wav);
        r->wav = malloc(r->wav_bytes ? r->wav_bytes : 1);
        if (!r->wav || r->served != 0 ||
            hipMemcpy(r->wav, r->d_wav, r->wav_bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return 0;
        t_line(&t_mark, "payload to the host");
        r->served = r->frames;
        *payload = r->wav;
        return r->wav_bytes;
    }
    free(r->wav);
    r->wav = malloc(bytes);
    if (!r->wav || !dev_alloc((void **)&d_out, bytes))
        return 0;
    /* planar: planes start at r->served inside each channel (shifted base, same stride);
     * frame-major: the values already are in payload order = one "channel" of left * channels values */
    const int rc = r->interleaved
        ? dvda_mlp_hip_pack_wav(r->d_pcm + r->served * r->channels, 4, 1, left * r->channels, bits, d_out, NULL)
        : dvda_mlp_hip_pack_wav(r->d_pcm + r->served, r->stride, r->channels, left, bits, d_out, NULL);
    if (rc != DVDA_HIP_OK ||
        hipMemcpy(r->wav, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipFree(d_out);
        return 0;
    }
    (void)hipFree(d_out);
    r->served = r->frames;
    *payload = r->wav;
    return bytes;
}
