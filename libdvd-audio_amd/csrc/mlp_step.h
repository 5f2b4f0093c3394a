/* mlp_step.h -- between mlp_stream.c (tier B, the mlp.h mirror: plain C) and mlp_stepper.h (a part of mlp_hip.hip): decoders whose state
 * stays on the device from one packet to the next.  Internal to the library (tier B is the public face:
 * include/dvda_mlp_hip.h, dvda_hip_mlpdecoder_decode_packet and dvda_hip_mlpdecoder_group_decode_packets).
 *
 * A stepper serves n members (decoders that share nothing; a lone decoder is n = 1).  One step = the whole access units
 * of one packet of every member that has some: bytes into the members' slots of one pinned region, parity / CRC-8
 * (k_step_check: workgroup i sums and joins member i's bytes, mlp_check.h), k_coop<false, true> (mlp_coop.h) with
 * workgroup i on member i -- it takes the decoder state from the device record (reference struct substream + filter
 * histories, src/mlp.c:103-115, 297-304), decodes the units and puts the state back -- PCM and a result record per member
 * into a second pinned region.  Two launches and one synchronise, however many members take part.  Nothing in front of
 * a packet is decoded again.
 *
 * Pinned host memory per member, allocated when the stepper is made: DVDA_STEP_SLOT_IN_BYTES on the way in (100 bytes
 * of descriptors beside it), DVDA_STEP_SLOT_OUT_BYTES on the way out -- 48.1 KB and 180.4 KB, 58.5 MB for 256 members. */
#ifndef DVDA_MLP_STEP_H
#define DVDA_MLP_STEP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DVDA_STEP_MAX_BYTES 49152u      /* one step's access units: at most this many bytes ... */
#define DVDA_STEP_MAX_UNITS 48u         /* ... and this many units (a caller with more steps more than once) */

#define DVDA_STEP_MAX_MEMBERS 256u      /* members of one stepper (DVDA_STREAM_GROUP_MAX): a workgroup per CU */
/* a member's bytes + the 128 zero bytes behind them (a multiple of 128: every slot starts where the checks' 128-byte
 * blocks do); its result record (400 bytes, padded) + 48 units x 160 frames x 6 channels of int32 */
#define DVDA_STEP_SLOT_IN_BYTES (DVDA_STEP_MAX_BYTES + 128u)
#define DVDA_STEP_SLOT_OUT_BYTES (512u + DVDA_STEP_MAX_UNITS * 160u * 6u * 4u)

typedef struct dvda_mlp_hip_stepper dvda_mlp_hip_stepper;

typedef struct {
    uint32_t status;        /* DVDA_ST_* of this step's access units */
    uint32_t frames_out;    /* access units that yielded PCM (a unit with a foreign major sync yields none) */
    uint32_t rows_written;  /* PCM frames per channel */
    uint32_t sync_seen;     /* 1 + index of the step's last unit that carries the stream's own major sync, 0: none */
    int32_t fir[2][48];     /* FIR histories in front of that unit, [substream][slot * 8 + tap] */
} dvda_mlp_step_result;

/* one member's part in a step: what goes in, and (rc == DVDA_HIP_OK) what came out */
typedef struct {
    uint32_t member;        /* which of the stepper's members (each at most once per step) */
    const uint8_t *bytes;   /* n_units whole access units (len even, <= DVDA_STEP_MAX_BYTES; n_units <= DVDA_STEP_MAX_UNITS) */
    size_t len;
    uint32_t n_units;
    uint32_t packed_sync;   /* the stream's latched major sync (g0 bps | g1 bps << 4 | g0 rate << 8 | g1 rate << 12 |
                               assignment << 16 | substreams << 24) */
    int fresh;              /* != 0: the first step of this member's decoder (no state yet) */
    int rc;                 /* DVDA_HIP_OK: took part; DVDA_HIP_EINVAL / DVDA_HIP_ECAPACITY: not what a step takes (left out) */
    const dvda_mlp_step_result *res;    /* host, valid until the member's next step; decode conditions in res->status */
    const int32_t *pcm;     /* planar int32 [channel][stride] in RIFF order (host, pinned), valid as res is */
    uint64_t stride;
    unsigned channels;
} dvda_mlp_step_item;

/* n: 1 .. DVDA_STEP_MAX_MEMBERS */
int dvda_mlp_hip_stepper_create(dvda_mlp_hip_stepper **out, unsigned n, int device);
void dvda_mlp_hip_stepper_destroy(dvda_mlp_hip_stepper *s);
/* One step for items[0, n_items): one k_step_check launch, one k_coop<false, true> launch, one synchronise.  Every item
 * gets its rc; the members of the items with rc == DVDA_HIP_OK were decoded, the others' state is untouched.  Returns
 * DVDA_HIP_OK (also when no item took part: nothing is launched then), DVDA_HIP_EINVAL for a bad argument, or the
 * DVDA_HIP_E* code of a HIP runtime failure, which concerns every item that took part. */
int dvda_mlp_hip_stepper_step(dvda_mlp_hip_stepper *s, dvda_mlp_step_item *items, unsigned n_items);

#ifdef __cplusplus
}
#endif
#endif
