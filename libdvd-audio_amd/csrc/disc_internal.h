/* disc_internal.h -- what the two halves of the disc tier share: disc_ifo.c (the IFO walk, the AOB files, the code
 * tables; host only, no HIP header) and disc_reader.c (the track readers).  Nothing here is exported. */
#ifndef DVDA_DISC_INTERNAL_H
#define DVDA_DISC_INTERNAL_H

#include <stdint.h>
#include <stdio.h>

#include "../../include/dvd-audio-hip.h"

#define SECTOR 2048u
#define MAX_AOBS 9
#define DISC_LOCAL __attribute__((visibility("hidden")))

struct track_span {
    unsigned pts_index, pts_length, first, last;
};

struct DVDA_Track_s {
    char *dir;
    unsigned titleset, title, number;
    struct track_span s;
};

/* the titleset's AOB files as one run of sectors (src/aob.c:86-127, 177-216) */
struct aob_set {
    FILE *f[MAX_AOBS];
    unsigned sectors[MAX_AOBS];
    unsigned n, total;
};

DISC_LOCAL void aob_open_all(struct aob_set *a, const char *dir, unsigned titleset);
DISC_LOCAL void aob_close_all(struct aob_set *a);
/* reads sectors [first, first + count) into dst; returns the number read (short at the end) */
DISC_LOCAL unsigned aob_read(struct aob_set *a, unsigned first, unsigned count, uint8_t *dst);

/* code tables (src/dvd-audio.c:1423-1496) */
DISC_LOCAL unsigned bits_of(unsigned code);
DISC_LOCAL unsigned rate_of(unsigned code);
DISC_LOCAL unsigned channels_of(unsigned assignment);

static inline unsigned be16(const uint8_t *p) { return ((unsigned)p[0] << 8) | p[1]; }

#endif
