/* disc_ifo.c -- the disc tier's host half (include/dvd-audio-hip.h): the disc, title set, title and track entry
 * points.  Plain C, no HIP header; built into libdvd_audio_hip.so with disc_reader.c (the track readers).
 *
 * Mirrors what reference src/dvd-audio.c + src/aob.c + src/audio_ts.c do:
 *
 *   IFO tables          parsed on the host, field for field (src/dvd-audio.c:896-1014)
 *   track sector range  dvda_open_title's rules (src/dvd-audio.c:426-492)
 *   AOB files           ATS_XX_1..9.AOB taken as one sector sequence (src/aob.c:86-190)
 */
#include <ctype.h>
#include <dirent.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "disc_internal.h"

/* ------------------------------------------------------------------ records */
struct ifo_title {
    unsigned track_count, index_count, pts_length;
    struct {
        unsigned index_number, pts_index, pts_length;
    } track[256];
    struct {
        unsigned first, last;
    } index[256];
};

struct DVDA_s {
    char *dir;
    unsigned titlesets;
};

struct DVDA_Titleset_s {
    char *dir;
    unsigned number, title_count;
    struct ifo_title *title;
};

struct DVDA_Title_s {
    char *dir;
    unsigned titleset, number, track_count, pts_length;
    struct track_span t[256];
};

/* ------------------------------------------------------------------ files */
static int same_name(const char *a, const char *b)
{
    for (; *a && *b; a++, b++)
        if (toupper((unsigned char)*a) != toupper((unsigned char)*b))
            return 0;
    return *a == *b;
}

/* case-insensitive lookup inside the AUDIO_TS directory (src/audio_ts.c:37-73) */
static char *find_file(const char *dir, const char *name)
{
    DIR *d = opendir(dir);
    struct dirent *e;
    char *path = NULL;
    if (!d)
        return NULL;
    while ((e = readdir(d)) != NULL) {
        if (same_name(name, e->d_name)) {
            const size_t n = strlen(dir) + 1 + strlen(e->d_name) + 1;
            path = malloc(n);
            if (path)
                snprintf(path, n, "%s/%s", dir, e->d_name);
            break;
        }
    }
    closedir(d);
    return path;
}

static unsigned be32(const uint8_t *p)
{
    return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3];
}

static uint8_t *slurp(const char *path, size_t *size)
{
    FILE *f = fopen(path, "rb");
    uint8_t *buf = NULL;
    long n;
    if (!f)
        return NULL;
    if (fseek(f, 0, SEEK_END) == 0 && (n = ftell(f)) >= 0 && fseek(f, 0, SEEK_SET) == 0) {
        buf = malloc((size_t)n + 1);
        if (buf && fread(buf, 1, (size_t)n, f) != (size_t)n) {
            free(buf);
            buf = NULL;
        }
        *size = (size_t)n;
    }
    fclose(f);
    return buf;
}

void aob_close_all(struct aob_set *a)
{
    for (unsigned i = 0; i < a->n; i++)
        fclose(a->f[i]);
    a->n = 0;
}

void aob_open_all(struct aob_set *a, const char *dir, unsigned titleset)
{
    memset(a, 0, sizeof(*a));
    for (unsigned k = 1; k <= MAX_AOBS; k++) {
        char name[16];
        char *path;
        struct stat st;
        snprintf(name, sizeof(name), "ATS_%2.2u_%1.1u.AOB", titleset % 100, k);
        path = find_file(dir, name);
        if (!path)
            break;
        if (stat(path, &st) != 0 || (a->f[a->n] = fopen(path, "rb")) == NULL) {
            free(path);
            break;
        }
        free(path);
        a->sectors[a->n] = (unsigned)(st.st_size / SECTOR);
        a->total += a->sectors[a->n];
        a->n++;
    }
}

unsigned aob_read(struct aob_set *a, unsigned first, unsigned count, uint8_t *dst)
{
    unsigned done = 0, base = 0;
    for (unsigned i = 0; i < a->n && done < count; i++) {
        const unsigned lo = base, hi = base + a->sectors[i];
        base = hi;
        if (first + done >= hi)
            continue;
        const unsigned at = first + done - lo;
        unsigned take = a->sectors[i] - at;
        if (take > count - done)
            take = count - done;
        if (fseek(a->f[i], (long)at * (long)SECTOR, SEEK_SET) != 0)
            break;
        const size_t got = fread(dst + (size_t)done * SECTOR, SECTOR, take, a->f[i]);
        done += (unsigned)got;
        if (got != take)
            break;
    }
    return done;
}

/* ------------------------------------------------------------------ disc / titleset / title / track */
DVDA *dvda_open(const char *audio_ts_path, const char *device)
{
    (void)device;               /* CPPM is not handled */
    if (!audio_ts_path)
        return NULL;
    char *ifo = find_file(audio_ts_path, "AUDIO_TS.IFO");
    if (!ifo)
        return NULL;
    size_t n = 0;
    uint8_t *b = slurp(ifo, &n);
    free(ifo);
    /* "DVDAUDIO-AMG", title set count in byte 63; the reference parses 104 bytes (src/dvd-audio.c:908-913) */
    unsigned count = 0;
    if (b && n >= 104 && memcmp(b, "DVDAUDIO-AMG", 12) == 0)
        count = b[63];
    free(b);
    if (!count)
        return NULL;
    DVDA *d = calloc(1, sizeof(*d));
    if (!d)
        return NULL;
    d->dir = strdup(audio_ts_path);
    d->titlesets = count;
    return d;
}

void dvda_close(DVDA *d)
{
    if (d) {
        free(d->dir);
        free(d);
    }
}

unsigned dvda_titleset_count(const DVDA *d) { return d->titlesets; }

/* one title table of ATS_XX_0.IFO (src/dvd-audio.c:975-1014); returns 0 when it leaves the file */
static int parse_title(const uint8_t *b, size_t n, size_t table, struct ifo_title *t)
{
    if (table + 16 > n)
        return 0;
    t->track_count = b[table + 2];
    t->index_count = b[table + 3];
    t->pts_length = be32(b + table + 4);
    const unsigned ptr_off = be16(b + table + 12);
    size_t p = table + 16;
    for (unsigned i = 0; i < t->track_count; i++, p += 20) {
        if (p + 20 > n)
            return 0;
        t->track[i].index_number = b[p + 4];
        t->track[i].pts_index = be32(b + p + 6);
        t->track[i].pts_length = be32(b + p + 10);
    }
    p = table + ptr_off;
    for (unsigned i = 0; i < t->index_count; i++, p += 12) {
        if (p + 12 > n)
            return 0;
        t->index[i].first = be32(b + p + 4);
        t->index[i].last = be32(b + p + 8);
    }
    return 1;
}

DVDA_Titleset *dvda_open_titleset(DVDA *d, unsigned titleset)
{
    char name[16];
    snprintf(name, sizeof(name), "ATS_%2.2u_0.IFO", titleset > 99 ? 99u : titleset);
    char *path = find_file(d->dir, name);
    if (!path)
        return NULL;
    size_t n = 0;
    uint8_t *b = slurp(path, &n);
    free(path);
    if (!b)
        return NULL;
    DVDA_Titleset *ts = NULL;
    if (n >= SECTOR + 8 && memcmp(b, "DVDAUDIO-ATS", 12) == 0) {
        ts = calloc(1, sizeof(*ts));
        ts->number = titleset;
        ts->title_count = be16(b + SECTOR);
        ts->title = calloc(ts->title_count ? ts->title_count : 1, sizeof(*ts->title));
        int ok = ts->title != NULL;
        for (unsigned i = 0; ok && i < ts->title_count; i++) {
            const size_t e = SECTOR + 8 + (size_t)8 * i;       /* title number 8u, 24p, table offset 32u */
            ok = e + 8 <= n && parse_title(b, n, SECTOR + (size_t)be32(b + e + 4), &ts->title[i]);
        }
        if (!ok) {
            free(ts->title);
            free(ts);
            ts = NULL;
        } else {
            ts->dir = strdup(d->dir);
        }
    }
    free(b);
    return ts;
}

void dvda_close_titleset(DVDA_Titleset *ts)
{
    if (ts) {
        free(ts->dir);
        free(ts->title);
        free(ts);
    }
}

unsigned dvda_titleset_number(const DVDA_Titleset *ts) { return ts->number; }
unsigned dvda_title_count(const DVDA_Titleset *ts) { return ts->title_count; }

static const unsigned *index_of(const struct ifo_title *t, unsigned track, int want_last)
{
    static const unsigned zero = 0;
    const unsigned k = t->track[track].index_number;
    if (k == 0 || k > 256)
        return &zero;
    return want_last ? &t->index[k - 1].last : &t->index[k - 1].first;
}

DVDA_Title *dvda_open_title(DVDA_Titleset *ts, unsigned title)
{
    if (title == 0 || title > ts->title_count)
        return NULL;
    const struct ifo_title *it = &ts->title[title - 1];
    DVDA_Title *t = calloc(1, sizeof(*t));
    if (!t)
        return NULL;
    t->dir = strdup(ts->dir);
    t->titleset = ts->number;
    t->number = title;
    t->track_count = it->track_count;
    t->pts_length = it->pts_length;
    for (unsigned i = 0; i < it->track_count; i++) {
        t->t[i].pts_index = it->track[i].pts_index;
        t->t[i].pts_length = it->track[i].pts_length;
        t->t[i].first = *index_of(it, i, 0);
        const unsigned own_last = *index_of(it, i, 1);
        /* a track runs up to the sector before the next track (of this or the next title);
         * only the very last one ends where its own index says (src/dvd-audio.c:452-488) */
        if (i + 1 < it->track_count) {
            t->t[i].last = *index_of(it, i + 1, 0) - 1;
        } else if (title < ts->title_count && ts->title[title].track_count) {
            const unsigned next_first = *index_of(&ts->title[title], 0, 0) - 1;
            t->t[i].last = next_first > own_last ? next_first : own_last;
        } else {
            t->t[i].last = own_last;
        }
    }
    return t;
}

void dvda_close_title(DVDA_Title *t)
{
    if (t) {
        free(t->dir);
        free(t);
    }
}

unsigned dvda_title_number(const DVDA_Title *t) { return t->number; }
unsigned dvda_track_count(const DVDA_Title *t) { return t->track_count; }
unsigned dvda_title_pts_length(const DVDA_Title *t) { return t->pts_length; }

DVDA_Track *dvda_open_track(DVDA_Title *t, unsigned track)
{
    if (track == 0 || track > t->track_count)
        return NULL;
    DVDA_Track *k = calloc(1, sizeof(*k));
    if (!k)
        return NULL;
    k->dir = strdup(t->dir);
    k->titleset = t->titleset;
    k->title = t->number;
    k->number = track;
    k->s = t->t[track - 1];
    return k;
}

void dvda_close_track(DVDA_Track *k)
{
    if (k) {
        free(k->dir);
        free(k);
    }
}

unsigned dvda_track_number(const DVDA_Track *k) { return k->number; }
unsigned dvda_track_pts_index(const DVDA_Track *k) { return k->s.pts_index; }
unsigned dvda_track_pts_length(const DVDA_Track *k) { return k->s.pts_length; }
unsigned dvda_track_first_sector(const DVDA_Track *k) { return k->s.first; }
unsigned dvda_track_last_sector(const DVDA_Track *k) { return k->s.last; }

/* ------------------------------------------------------------------ code tables (src/dvd-audio.c:1423-1496) */
unsigned bits_of(unsigned code) { return code == 0 ? 16 : code == 1 ? 20 : code == 2 ? 24 : 0; }

unsigned rate_of(unsigned code)
{
    switch (code) {
    case 0: return 48000;
    case 1: return 96000;
    case 2: return 192000;
    case 8: return 44100;
    case 9: return 88200;
    case 10: return 176400;
    default: return 0;
    }
}

unsigned channels_of(unsigned assignment)
{
    static const uint8_t n[21] = {1, 2, 3, 4, 3, 4, 5, 3, 4, 5, 4, 5, 6, 4, 5, 4, 5, 6, 5, 5, 6};
    return assignment < 21 ? n[assignment] : 0;
}

