/* dvda2wav_hip -- extracts the tracks of a DVD-Audio disc to WAV files on the GPU.
 *
 * Same command line and the same output files (names, 68-byte WAVE_FORMAT_EXTENSIBLE header,
 * data bytes) as the reference's utility (reference utils/dvda2wav.c:57-186, 257-397), built on
 * libdvd_audio_hip.so only: IFO walk, sector demux, MLP decode / PCM un-swizzle and the
 * write_signed packing of the data chunk all run through include/dvd-audio-hip.h; this file does
 * argument parsing, the header and fwrite().
 *
 *   cc -O2 -o dvda2wav_hip tools/dvda2wav_hip.c -Iinclude -Llibdvd-audio_amd -ldvd_audio_hip \
 *      -ldvda_mlp_hip -Wl,-rpath,'$ORIGIN/../libdvd-audio_amd'
 */
#include <getopt.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "dvd-audio-hip.h"
#include "dvda_mlp_hip.h"           /* struct dvda_mlp_conceal_span (--conceal) */

static void put16(uint8_t *p, unsigned v) { p[0] = v & 0xFF; p[1] = (v >> 8) & 0xFF; }
static void put32(uint8_t *p, unsigned v) { put16(p, v & 0xFFFF); put16(p + 2, v >> 16); }

/* RIFF/WAVE_FORMAT_EXTENSIBLE header as the reference writes it (utils/dvda2wav.c:352-397):
 * note that its RIFF size field counts the 12 + 8 + 40 + 8 header bytes themselves */
static void wave_header(uint8_t h[68], unsigned rate, unsigned channels, unsigned mask, unsigned bits,
                        unsigned frames)
{
    static const uint8_t guid[16] = {1, 0, 0, 0, 0, 0, 16, 0, 128, 0, 0, 170, 0, 56, 155, 113};
    const unsigned bytes = bits / 8, data = bytes * channels * frames;
    memcpy(h, "RIFF", 4);
    put32(h + 4, 12 + 40 + 8 + data + (data % 2));
    memcpy(h + 8, "WAVEfmt ", 8);
    put32(h + 16, 40);
    put16(h + 20, 0xFFFE);
    put16(h + 22, channels);
    put32(h + 24, rate);
    put32(h + 28, rate * channels * bytes);
    put16(h + 32, channels * bytes);
    put16(h + 34, bits);
    put16(h + 36, 22);
    put16(h + 38, bits);
    put32(h + 40, mask);
    memcpy(h + 44, guid, 16);
    memcpy(h + 60, "data", 4);
    put32(h + 64, data);
}

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

/* -b / --dither / --seed: the word length every track is delivered at (0: its own), set once before any worker starts */
static unsigned g_rq_bits, g_rq_mode = DVDA_RQ_TPDF;
static unsigned long long g_rq_seed;
/* -r: the rate every track is delivered at where its own is 1, 2 or 4 times that (0: its own) */
static unsigned g_rate;
/* --resample: with -r 44100, a 48 / 96 / 192 kHz track is resampled to 44.1 kHz */
static int g_resample;
/* --downmix: the channels every track of another count is mixed to (0: its own), and the DVDA_MIX_* flags */
static unsigned g_mix_ch, g_mix_flags;

static int extract(DVDA_Title *title, unsigned track_num, const char *dir, int device, int fused_wav, int stereo,
                   int crc, int conceal, unsigned titleset_num)
{
    const int timing = getenv("DVDA_TOOL_TIMING") != NULL;       /* diagnostic: where a track's wall-clock time goes */
    const double t_begin = now_s();
    double t_write = 0;
    DVDA_Track *track = dvda_open_track(title, track_num);
    if (!track) {
        fprintf(stderr, "*** Error: unable to open track %u\n", track_num);
        return 0;
    }
    /* this tool only ever writes WAV files: MLP tracks are decoded straight into the payload */
    /* --stereo: a two-substream MLP track comes out as the 2-channel presentation its substream 0 carries */
    /* --crc: the reader digests the track on the device, before the payload is copied (read when the reader is opened) */
    dvda_hip_set_digest(crc);
    /* --conceal: a damaged MLP track is written with silence where the damage is, not refused (an explicit choice either
       way: the tool's option decides, not DVDA_CONCEAL in the environment) */
    dvda_hip_set_conceal(conceal);
    /* -b: the reader reduces the track to that word length on the device; its depth is then the file's */
    dvda_hip_set_requantize(g_rq_bits, g_rq_mode, g_rq_seed);
    /* -r: the reader decimates the track by its rate / RATE on the device.  The rate is the stream's own and is known once
       a reader is open: the first one is opened by 2 (96 -> 48, 88.2 -> 44.1: the common case; a track that cannot be
       divided by 2 comes as it is), and where that did not give RATE the track is opened again, by 4 or as it is.  A
       track long enough to be read in windows is refused by 2: it is opened as it is to learn its rate, and fails only
       where it really needs a ratio */
    /* --downmix: the reader mixes the track to one or two channels on the device, in front of all of that */
    dvda_hip_set_downmix(g_mix_ch, g_mix_flags);
    dvda_hip_set_decimate(g_rate ? 2 : 0);
    DVDA_Track_Reader *r = dvda_hip_open_track_reader_with(track, device, fused_wav, stereo);
    if (g_rate && (!r || dvda_sample_rate(r) != g_rate)) {
        const int refused = !r;
        if (refused) {
            dvda_hip_set_decimate(0);
            r = dvda_hip_open_track_reader_with(track, device, fused_wav, stereo);
        }
        const unsigned src = dvda_hip_reader_source_rate(r);
        const unsigned ratio = src == 2 * g_rate ? 2 : src == 4 * g_rate ? 4 : 0;
        /* (--resample takes the 48 kHz family below) */
        if (r && src != g_rate && !ratio && !(g_resample && (src == 48000 || src == 96000 || src == 192000)))
            fprintf(stderr, "*** Warning: track %u runs at %u Hz, which is not 1, 2 or 4 times %u: written as it is\n", track_num,
                    src, g_rate);
        if (r && (ratio || dvda_hip_reader_decimated(r, NULL) == 1)) {
            dvda_close_track_reader(r);
            dvda_hip_set_decimate(ratio);
            r = refused && ratio == 2 ? NULL : dvda_hip_open_track_reader_with(track, device, fused_wav, stereo);
            if (!r && refused)
                fprintf(stderr, "*** Error: track %u runs at %u Hz and is read in windows: -r cannot divide it by %u\n", track_num,
                        src, ratio);
        }
    }
    dvda_hip_set_decimate(0);
    /* --resample: a track that came out at its own rate in the 48 kHz family is opened once more, resampled */
    if (g_resample && r && dvda_sample_rate(r) != g_rate && dvda_hip_reader_decimated(r, NULL) != 1) {
        const unsigned src = dvda_sample_rate(r);
        if (src == 48000 || src == 96000 || src == 192000) {
            const int windowed = dvda_hip_reader_windowed(r);
            dvda_close_track_reader(r);
            dvda_hip_set_resample(g_rate);
            r = windowed ? NULL : dvda_hip_open_track_reader_with(track, device, fused_wav, stereo);
            dvda_hip_set_resample(0);
            if (!r)
                fprintf(stderr, "*** Error: track %u runs at %u Hz%s: --resample cannot bring it to %u\n", track_num, src,
                        windowed ? " and is read in windows" : "", g_rate);
        }
    }
    dvda_hip_set_downmix(0, 0);
    if (!r) {
        fprintf(stderr, "*** Error: unable to open track %u for reading\n", track_num);
        dvda_close_track(track);
        return 0;
    }
    const double t_opened = now_s();
    char path[4096];
    const size_t n = strlen(dir);
    const unsigned title_number = dvda_title_number(title), track_number = dvda_track_number(track);
    snprintf(path, sizeof(path), "%s%strack-%2.2u-%2.2u.wav", dir, n && dir[n - 1] == '/' ? "" : "/", title_number,
             track_number);
    dvda_close_track(track);
    FILE *f = fopen(path, "wb");
    if (!f) {
        fprintf(stderr, "*** Error: unable to open \"%s\" for writing\n", path);
        dvda_close_track_reader(r);
        return 0;
    }
    const unsigned channels = dvda_channel_count(r), bits = dvda_bits_per_sample(r), rate = dvda_sample_rate(r);
    printf("* Extracting %s track  %u channels  %u Hz  %u bps\n", dvda_codec(r) == DVDA_MLP ? "MLP" : "PCM",
           channels, rate, bits);
    /* the header first, as the reference does (utils/dvda2wav.c:316-343: a placeholder, the data chunk as it is read, the
       finished header written over it) -- a long track comes window by window and knows its length at its end; a short
       one hands out its whole payload as the one and only piece */
    uint8_t h[68];
    const unsigned mask = dvda_riff_wave_channel_mask(r);
    wave_header(h, rate, channels, mask, bits, 0);
    int ok = fwrite(h, 1, sizeof(h), f) == sizeof(h);
    unsigned long long bytes = 0, piece;
    const unsigned char *payload = NULL;
    while (ok && (piece = dvda_hip_reader_wav_next(r, &payload)) != 0) {
        const double tw = now_s();
        ok = fwrite(payload, 1, piece, f) == piece;
        t_write += now_s() - tw;
        bytes += piece;
    }
    const double t_pieces = now_s();
    const unsigned long long frames = dvda_hip_reader_total_frames(r);
    if (dvda_hip_reader_windowed(r)) {
        /* a track read in windows: what it held at most (tools/disc_bench.py reads this line) */
        unsigned long long hp = 0, dp = 0;
        dvda_hip_reader_memory(r, &hp, &dp);
        printf("* Read in windows: host peak %.1f MB, device peak %.1f MB, payload %.1f MB\n", hp / 1e6, dp / 1e6, bytes / 1e6);
    }
    if (ok) {
        wave_header(h, rate, channels, mask, bits, (unsigned)frames);
        ok = fseek(f, 0, SEEK_SET) == 0 && fwrite(h, 1, sizeof(h), f) == sizeof(h);
    }
    ok = fclose(f) == 0 && ok;
    /* (a window that could not be read or decoded ends the pieces early: that is a failed track, not a short one) */
    ok = ok && bytes == frames * channels * (bits / 8) && !dvda_hip_reader_failed(r);
    if (ok && crc) {
        /* final once the track has been read to its end: the CRC-32 of the data chunk just written */
        unsigned v = 0;
        unsigned long long vb = 0;
        if (dvda_hip_reader_crc32(r, &v, &vb) == 1)
            printf("CRC32 %u %u %u %08x %llu\n", titleset_num, title_number, track_number, v, vb);
        else
            printf("CRC32 %u %u %u none 0\n", titleset_num, title_number, track_number);
    }
    if (ok && g_rq_bits) {
        /* what the reduction did to the track just written: source depth, the file's depth, values the clamp changed */
        struct dvda_pcm_requant_report rq;
        if (dvda_hip_reader_requantized(r, &rq) == 1) {
            unsigned long long clipped = 0;
            for (int c = 0; c < 8; c++)
                clipped += rq.clipped[c];
            printf("REQUANT %u %u %u %u %u %llu\n", titleset_num, title_number, track_number, dvda_hip_reader_source_bits(r),
                   bits, clipped);
        } else {
            printf("REQUANT %u %u %u %u %u none\n", titleset_num, title_number, track_number, dvda_hip_reader_source_bits(r),
                   bits);
        }
    }
    if (ok && g_rate) {
        /* what the decimation did to the track just written: the rate on the disc, the file's rate, values the clamp changed */
        struct dvda_pcm_decim_report dc;
        if (dvda_hip_reader_decimated(r, &dc) == 1) {
            unsigned long long clipped = 0;
            for (int c = 0; c < 8; c++)
                clipped += dc.clipped[c];
            printf("DECIMATE %u %u %u %u %u %llu\n", titleset_num, title_number, track_number, dvda_hip_reader_source_rate(r),
                   rate, clipped);
        } else {
            printf("DECIMATE %u %u %u %u %u none\n", titleset_num, title_number, track_number, dvda_hip_reader_source_rate(r),
                   rate);
        }
    }
    if (ok && g_mix_ch) {
        /* what the mix did to the track just written: the channels on the disc, the file's, values the clamp changed */
        struct dvda_pcm_mix_report mx;
        if (dvda_hip_reader_downmixed(r, &mx) == 1) {
            unsigned long long clipped = 0;
            for (int c = 0; c < 8; c++)
                clipped += mx.clipped[c];
            printf("DOWNMIX %u %u %u %u %u %llu\n", titleset_num, title_number, track_number,
                   dvda_hip_reader_source_channels(r), dvda_channel_count(r), clipped);
        } else {
            printf("DOWNMIX %u %u %u %u %u none\n", titleset_num, title_number, track_number,
                   dvda_hip_reader_source_channels(r), dvda_channel_count(r));
        }
    }
    if (ok && g_resample) {
        /* what the resampler did to the track just written: the rate on the disc, the file's rate, values the clamps changed
           (those of the decimation in front of it included) */
        struct dvda_pcm_decim_report rs, dc;
        if (dvda_hip_reader_resampled(r, &rs) == 1) {
            unsigned long long clipped = 0;
            const int staged = dvda_hip_reader_decimated(r, &dc) == 1;
            for (int c = 0; c < 8; c++)
                clipped += rs.clipped[c] + (staged ? dc.clipped[c] : 0);
            printf("RESAMPLE %u %u %u %u %u %llu\n", titleset_num, title_number, track_number, dvda_hip_reader_source_rate(r),
                   rate, clipped);
        } else {
            printf("RESAMPLE %u %u %u %u %u none\n", titleset_num, title_number, track_number, dvda_hip_reader_source_rate(r),
                   rate);
        }
    }
    if (ok && conceal) {
        /* what was concealed of the track just written: one line per span */
        unsigned n_spans = 0;
        if (dvda_hip_reader_concealed(r, NULL, 0, &n_spans) == 1 && n_spans) {
            struct dvda_mlp_conceal_span *sp = malloc(n_spans * sizeof(*sp));
            if (sp && dvda_hip_reader_concealed(r, sp, n_spans, &n_spans) == 1)
                for (unsigned i = 0; i < n_spans; i++)
                    printf("CONCEALED %u %u %u %llu %llu %llu %llu %x %u\n", titleset_num, title_number, track_number,
                           (unsigned long long)sp[i].first_frame, (unsigned long long)sp[i].frames,
                           (unsigned long long)sp[i].byte_off, (unsigned long long)sp[i].byte_end, sp[i].cause, sp[i].flags);
            free(sp);
        }
    }
    if (ok)
        printf("* Wrote: \"%s\"\n", path);
    else
        fprintf(stderr, "*** Error: writing \"%s\"\n", path);
    dvda_close_track_reader(r);
    if (timing)
        fprintf(stderr, "timing: track %u  open %.1f ms  pieces %.1f ms (of which fwrite %.1f)  finish %.1f ms  at %.1f ms\n", track_num,
                (t_opened - t_begin) * 1e3, (t_pieces - t_opened) * 1e3, t_write * 1e3, (now_s() - t_pieces) * 1e3,
                now_s() * 1e3);
    return ok;
}

/* ---- tracks fanned out over device entries (SURVEY 8(e) from the C host: tracks are independent -- the reference
 *      extracts them one after the other through one decoder, utils/dvda2wav.c:287-350, src/dvd-audio.c:597-657):
 *      one worker thread per entry of --devices, each takes the next track of the job list, opens it on ITS device,
 *      fetches the payload and writes the file.  A device named more than once is that many workers on it: one
 *      worker's file read and WAV write overlap another's decode. */
struct job {
    DVDA_Title *title;
    unsigned track;
};
struct pool {
    struct job *jobs;
    unsigned n_jobs;
    atomic_uint next, failed, done;     /* done: workers through with the job list */
    const char *dir;
    int fused_wav;
    int stereo;                         /* --stereo: the 2-channel presentation of two-substream MLP tracks */
    int crc;                            /* --crc: one CRC32 line per track */
    int conceal;                        /* --conceal: damaged MLP tracks are concealed; one CONCEALED line per span */
    unsigned titleset;
    int park;                           /* a worker that is through parks instead of ending (the fast way out) */
};
struct worker {
    struct pool *pool;
    int device;
    int threaded;                       /* runs in a thread of its own (not in main's) */
};

static void *work(void *arg)
{
    struct worker *w = arg;
    for (;;) {
        const unsigned i = atomic_fetch_add(&w->pool->next, 1);
        if (i >= w->pool->n_jobs)
            break;
        if (!extract(w->pool->jobs[i].title, w->pool->jobs[i].track, w->pool->dir, w->device, w->pool->fused_wav, w->pool->stereo,
                     w->pool->crc, w->pool->conceal, w->pool->titleset))
            atomic_fetch_add(&w->pool->failed, 1);
    }
    /* (what this thread's last windowed reader left for a next one would be freed when the thread ends -- 30 ms a worker.
       main() does not wait for that: it leaves with _exit as soon as every worker is through with the list, and a worker
       that has counted itself done PARKS here instead of ending, so that no thread is inside a HIP call -- its buffers'
       release -- when the process goes.  DVDA_TOOL_FULL_TEARDOWN=1: the orderly way, threads joined, everything freed) */
    atomic_fetch_add(&w->pool->done, 1);
    if (w->pool->park && w->threaded)
        for (;;)
            pause();
    return NULL;
}

static void usage(const char *prog)
{
    printf("*** Usage : %s -A [AUDIO_TS] [OPTIONS]\n"
           "Options:\n"
           "  -h, --help                show this help message and exit\n"
           "  -A PATH, --audio_ts=PATH  path to disc's AUDIO_TS directory\n"
           "  -S SET, --titleset=SET    title set number (default 1)\n"
           "  -T TITLE, --title=TITLE   title number to extract (default: all)\n"
           "  -t TRACK, --track=TRACK   track number to extract (default: all)\n"
           "  -d DIR, --dir=DIR         output directory (default: the working directory)\n"
           "  -2, --stereo              write the 2-channel presentation of multichannel MLP tracks (substream 0\n"
           "                            alone: the stereo mix a 2-channel player plays), not all channels\n"
           "  -C, --crc                 print the CRC-32 (zlib) of every track's WAV data chunk, computed on the GPU, one\n"
           "                            line per track on stdout: CRC32 <titleset> <title> <track> <crc, 8 hex digits>\n"
           "                            <bytes> (\"none 0\" for a bit depth other than 16 / 24); -c is --cdrom\n"
           "  -K, --conceal             write a damaged MLP track with silence in place of the damage instead of failing\n"
           "                            on it; one line per concealed span on stdout: CONCEALED <titleset> <title> <track>\n"
           "                            <first_frame> <frames> <byte_off> <byte_end> <cause, hex> <flags>\n"
           "  -b BITS, --bits=BITS      deliver every track at BITS bits (16 or 24): reduced on the GPU, clamped where the\n"
           "                            plain payload would wrap; a track below BITS is written as it is.  One line per\n"
           "                            track on stdout: REQUANT <titleset> <title> <track> <source bits> <file's bits>\n"
           "                            <values clamped> (\"none\" for a track written as it is).  Not together with -K\n"
           "      --dither=MODE         none | round | tpdf (default): truncate, round, or triangular dither of +-1 LSB\n"
           "      --seed=N              seed of the dither's noise (default 0): the same seed gives the same file\n"
           "  -r RATE, --rate=RATE      deliver every track at RATE Hz (44100, 48000, 88200 or 96000) where its own rate is\n"
           "                            2 or 4 times that: filtered and decimated on the GPU, exact, clamped at the track's\n"
           "                            depth; any other track is written as it is, with a warning unless it runs at RATE.\n"
           "                            One line per track on stdout: DECIMATE <titleset> <title> <track> <source rate>\n"
           "                            <file's rate> <values clamped> (\"none\" for a track written as it is).  Composes\n"
           "                            with -b / --dither (the reduction follows the decimation).  Whole-track readers\n"
           "                            only: a track long enough to be read in windows fails where it would have to be\n"
           "                            decimated, and is written as it is where not.  Not together with -K\n"
           "      --downmix[=mono][,lfe][,unity]  mix every track of another channel count to 2 channels (mono: 1) on the\n"
           "                            GPU with the default matrix of its channel assignment, exact, clamped at the track's\n"
           "                            depth, in front of -r, --resample and -b; lfe: the LFE takes part; unity: the fronts\n"
           "                            at gain 1 (the default scales so that nothing clips).  One line per track on stdout:\n"
           "                            DOWNMIX <titleset> <title> <track> <source channels> <file's channels> <values\n"
           "                            clamped> (\"none\" for a track written as it is).  Whole-track readers only.  Not\n"
           "                            together with -K\n"
           "      --resample            with -r 44100: a 48, 96 or 192 kHz track is brought to 44100 Hz too (decimated by 2 or\n"
           "                            4 where its rate asks for it, then resampled by 147 / 160 on the GPU, exact, clamped\n"
           "                            at the track's depth).  One line per track on stdout: RESAMPLE <titleset> <title>\n"
           "                            <track> <source rate> <file's rate> <values clamped> (\"none\" for a track that was\n"
           "                            not resampled).  Whole-track readers only\n"
           "  -g N, --gpu=N             HIP device (default 0)\n"
           "  -D LIST, --devices=LIST   comma-separated HIP devices: one worker thread per entry takes tracks in turn\n"
           "                            (default: up to four workers on the device of -g)\n"
           "                            (a device may be named more than once)\n", prog);
}

int main(int argc, char *argv[])
{
    static struct option longopts[] = {{"audio_ts", required_argument, 0, 'A'}, {"cdrom", required_argument, 0, 'c'},
                                       {"titleset", required_argument, 0, 'S'}, {"title", required_argument, 0, 'T'},
                                       {"track", required_argument, 0, 't'},    {"dir", required_argument, 0, 'd'},
                                       {"gpu", required_argument, 0, 'g'},      {"help", no_argument, 0, 'h'},
                                       {"devices", required_argument, 0, 'D'},  {"stereo", no_argument, 0, '2'},
                                       {"crc", no_argument, 0, 'C'},            {"conceal", no_argument, 0, 'K'},
                                       {"bits", required_argument, 0, 'b'},     {"dither", required_argument, 0, 1001},
                                       {"seed", required_argument, 0, 1002},    {"rate", required_argument, 0, 'r'},
                                       {"resample", no_argument, 0, 1003},
                                       {"downmix", optional_argument, 0, 1004},
                                       {0, 0, 0, 0}};
    const char *audio_ts = NULL, *dir = ".", *cdrom = NULL;
    unsigned titleset_num = 1, title_num = 0, track_num = 0;
    int devices[64], n_devices = 0, one_device = 0, stereo = 0, crc = 0, conceal = 0;
    int c;
    if (getenv("DVDA_TOOL_TIMING"))
        fprintf(stderr, "timing: main at %.1f ms\n", now_s() * 1e3);
    while ((c = getopt_long(argc, argv, "A:c:S:T:t:d:g:D:b:r:h2CK", longopts, NULL)) != -1) {
        switch (c) {
        case 'A': audio_ts = optarg; break;
        case 'c': cdrom = optarg; break;
        case 'S': titleset_num = (unsigned)strtoul(optarg, NULL, 10); break;
        case 'T': title_num = (unsigned)strtoul(optarg, NULL, 10); break;
        case 't': track_num = (unsigned)strtoul(optarg, NULL, 10); break;
        case 'd': dir = optarg; break;
        case 'g': one_device = atoi(optarg); break;
        case 'D':
            for (char *tok = strtok(optarg, ","); tok && n_devices < 64; tok = strtok(NULL, ","))
                devices[n_devices++] = atoi(tok);
            break;
        case '2': stereo = 1; break;
        case 'C': crc = 1; break;
        case 'K': conceal = 1; break;
        case 'b': g_rq_bits = (unsigned)strtoul(optarg, NULL, 10); break;
        case 1001:
            if (!strcmp(optarg, "none"))
                g_rq_mode = DVDA_RQ_TRUNCATE;
            else if (!strcmp(optarg, "round"))
                g_rq_mode = DVDA_RQ_ROUND;
            else if (!strcmp(optarg, "tpdf"))
                g_rq_mode = DVDA_RQ_TPDF;
            else {
                fprintf(stderr, "*** Error: --dither takes none, round or tpdf\n");
                return 1;
            }
            break;
        case 'r': g_rate = (unsigned)strtoul(optarg, NULL, 10); break;
        case 1002: g_rq_seed = strtoull(optarg, NULL, 0); break;
        case 1003: g_resample = 1; break;
        case 1004:
            g_mix_ch = 2;
            for (char *tok = optarg ? strtok(optarg, ",") : NULL; tok; tok = strtok(NULL, ",")) {
                if (!strcmp(tok, "mono"))
                    g_mix_ch = 1;
                else if (!strcmp(tok, "stereo"))
                    g_mix_ch = 2;
                else if (!strcmp(tok, "lfe"))
                    g_mix_flags |= DVDA_MIX_LFE;
                else if (!strcmp(tok, "unity"))
                    g_mix_flags |= DVDA_MIX_UNITY;
                else {
                    fprintf(stderr, "*** Error: --downmix takes mono, lfe and unity, separated by commas\n");
                    return 1;
                }
            }
            break;
        case 'h': usage(argv[0]); return 0;
        default: return 1;
        }
    }
    if (!audio_ts) {
        usage(argv[0]);
        return 0;
    }
    if (g_rq_bits && ((g_rq_bits != 16 && g_rq_bits != 24) || conceal)) {
        fprintf(stderr, "*** Error: -b takes 16 or 24 (the depths a WAV payload has here), and not together with -K\n");
        return 1;
    }
    if (g_rate && ((g_rate != 44100 && g_rate != 48000 && g_rate != 88200 && g_rate != 96000) || conceal)) {
        fprintf(stderr, "*** Error: -r takes 44100, 48000, 88200 or 96000, and not together with -K\n");
        return 1;
    }
    if (g_mix_ch && conceal) {
        fprintf(stderr, "*** Error: --downmix does not go together with -K\n");
        return 1;
    }
    if (g_resample && g_rate != 44100) {
        fprintf(stderr, "*** Error: --resample goes with -r 44100\n");
        return 1;
    }
    /* (DVDA_NO_FUSED_WAV=1 in the environment brings the int32 decode + packing pass back, for comparison) */
    const int fused_wav = getenv("DVDA_NO_FUSED_WAV") == NULL;
    DVDA *dvda = dvda_open(audio_ts, cdrom);
    DVDA_Titleset *ts = dvda ? dvda_open_titleset(dvda, titleset_num) : NULL;
    if (!ts) {
        fprintf(stderr, "*** Error: \"%s\" does not appear to be a valid AUDIO_TS path\n", audio_ts);
        if (dvda)
            dvda_close(dvda);
        return 1;
    }
    int rc = 0;
    const unsigned t_lo = title_num ? title_num : 1, t_hi = title_num ? title_num : dvda_title_count(ts);
    /* the job list: every (title, track) asked for, in the reference tool's order */
    DVDA_Title *titles[256];
    unsigned n_titles = 0, n_jobs = 0, cap_jobs = 0;
    struct job *jobs = NULL;
    for (unsigned t = t_lo; t <= t_hi && !rc && n_titles < 256; t++) {
        DVDA_Title *title = dvda_open_title(ts, t);
        if (!title) {
            fprintf(stderr, "*** Error: unable to open title %u\n", t);
            rc = 1;
            break;
        }
        titles[n_titles++] = title;
        const unsigned k_lo = track_num ? track_num : 1, k_hi = track_num ? track_num : dvda_track_count(title);
        for (unsigned k = k_lo; k <= k_hi; k++) {
            if (n_jobs == cap_jobs) {
                cap_jobs = cap_jobs ? 2 * cap_jobs : 64;
                jobs = realloc(jobs, cap_jobs * sizeof(*jobs));
                if (!jobs)
                    return 1;
            }
            jobs[n_jobs].title = title;
            jobs[n_jobs++].track = k;
        }
    }
    if (n_devices == 0) {
        /* no --devices: a pool of up to four workers on the one device (-g, default 0) -- one worker's file read and
           WAV write overlap the others' decodes; a single track needs no pool */
        const unsigned w = n_jobs >= 4 ? 4 : (n_jobs ? n_jobs : 1);
        for (unsigned i = 0; i < w; i++)
            devices[n_devices++] = one_device;
    }
    struct pool pool = {jobs, n_jobs, 0, 0, 0, dir, fused_wav, stereo, crc, conceal, titleset_num, getenv("DVDA_TOOL_FULL_TEARDOWN") == NULL};
    struct worker workers[64];
    pthread_t th[64];
    int started[64];
    for (int i = 0; i < n_devices; i++) {
        workers[i].pool = &pool;
        workers[i].device = devices[i];
        workers[i].threaded = n_devices > 1;
        started[i] = n_devices > 1 && pthread_create(&th[i], NULL, work, &workers[i]) == 0;
        if (!started[i]) {
            workers[i].threaded = 0;
            work(&workers[i]);              /* one entry (or no thread to be had): here, in turn */
        }
    }
    {
        unsigned n_started = 0;
        for (int i = 0; i < n_devices; i++)
            n_started += started[i] ? 1u : 0u;
        if (getenv("DVDA_TOOL_FULL_TEARDOWN")) {
            for (int i = 0; i < n_devices; i++)
                if (started[i])
                    pthread_join(th[i], NULL);
        } else {
            /* every file is closed when a worker counts itself done; its buffers' release is not waited for */
            while (atomic_load(&pool.done) < n_started) {
                struct timespec ts = {0, 200000};
                nanosleep(&ts, NULL);
            }
        }
    }
    /* a track that could not be extracted (no such device, a read error, a decode the library reports) fails the run */
    if (atomic_load(&pool.failed)) {
        fprintf(stderr, "*** Error: %u of %u tracks could not be extracted\n", atomic_load(&pool.failed), n_jobs);
        rc = 1;
    }
    /* every file is written and closed.  What is left -- the titles' tables, and the HIP runtime's own teardown at exit
       (some 60-80 ms, measured: tools/probe/r05_disc_time.sh) -- is the operating system's to reclaim: a command-line
       tool that is done leaves */
    fflush(stdout);
    fflush(stderr);
    if (!getenv("DVDA_TOOL_FULL_TEARDOWN"))
        _exit(rc);
    for (unsigned i = 0; i < n_titles; i++)
        dvda_close_title(titles[i]);
    free(jobs);
    dvda_close_titleset(ts);
    dvda_close(dvda);
    return rc;
}
