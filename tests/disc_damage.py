"""Damaged MLP tracks for the disc tier's conceal mode (dvda_hip_set_conceal): the sectors of a track with damage applied
to them, and D -- the bytes the demux yields for them, cut as the track reader cuts its stream (csrc/disc_reader.c,
stream_bounds) -- which is what tests/conceal_model.conceal is asked about.

Damage, in sector terms (indices into disc.mlp_track_sectors(stream)):
    lost      sector indices that read as zeros: the scan kernel refuses them, they contribute nothing to D
    flips     (sector, body byte, xor mask): one byte of a sector's MLP payload changed inside a valid packet
    garbage   (first sector, count, seed): runs of sectors whose payload is random bytes inside valid packets
"""
import numpy as np

BODY = 2048 - 14 - 6 - 7        # MLP bytes a full sector carries (pack header, PES header, audio packet header)
PATTERN = b"\xF8\x72\x6F\xBB"


def damaged_sectors(disc, stream, lost=(), flips=(), garbage=()):
    """-> (sectors, bodies): the track's sectors with the damage applied, and per sector the MLP bytes the demux
    takes from it (None: the sector is refused)"""
    data = bytes(np.asarray(stream, np.uint8))
    bodies = [bytearray(data[off:off + BODY]) for off in range(0, len(data), BODY)]
    for first, count, seed in garbage:
        rng = np.random.RandomState(seed)
        for s in range(first, first + count):
            bodies[s] = bytearray(rng.randint(0, 256, len(bodies[s]), dtype=np.uint8).tobytes())
    for s, at, mask in flips:
        bodies[s][at] ^= mask
    lost = set(lost)
    sectors = [bytes(disc.SECTOR) if s in lost else disc._sector(disc.MLP_CODEC, bytes(b)) for s, b in enumerate(bodies)]
    return sectors, [None if s in lost else bytes(b) for s, b in enumerate(bodies)]


def find_sync(data, start):
    """offset of the first major-sync pattern (bytes +4..+7) at or after `start` whose 8 bytes lie inside data, or -1"""
    at = data.find(PATTERN, start + 4)
    return at - 4 if at >= 0 else -1


def track_stream(bodies, first, last):
    """D of the track that owns sectors [first, last] of a title set whose sectors carry `bodies`, by the reader's rule:
    from the first major-sync pattern of the track's payload to the first one at or behind the first payload byte of a
    sector beyond the track -- all of it when the title set ends with the track, 7 bytes short of the data when bytes
    follow but no sync does"""
    own = b"".join(b for b in bodies[first:last + 1] if b is not None)
    ahead = b"".join(b for b in bodies[last + 1:] if b is not None)
    data = own + ahead
    begin = find_sync(data, 0)
    assert begin >= 0, "no major sync in the track"
    end = len(data)
    if len(bodies) > last + 1:
        boundary = len(own)
        s1 = find_sync(data, max(boundary, begin))
        end = s1 if s1 >= 0 else (len(data) - 7 if len(data) - boundary >= 8 else boundary)
    return np.frombuffer(data[begin:end], np.uint8)


def damaged_track(disc, stream, lost=(), flips=(), garbage=()):
    """one track that is the whole title set -> (sectors, D)"""
    sectors, bodies = damaged_sectors(disc, stream, lost, flips, garbage)
    return sectors, track_stream(bodies, 0, len(bodies) - 1)
