"""The streaming tier's cases (csrc/mlp_stream.c, csrc/mlp_stepper.h, k_coop<false, true>), one table for the CPU file
(tests/test_streaming_model.py: the premises, on the oracle) and the GPU file (tests/test_gpu_streaming.py).

Every fixture is made from the generator, tests/stream_tools.py and nothing else, so both files see the same bytes:

    HANDOVER   streams that the stepping kernel decodes for many access units and then hands to the batch-tier path:
               a unit padded past the 4 KB stage (DVDA_ST_SEQ) or a tail of non-standard units (DVDA_ST_TIMING)
    BOUNDARY   rich-feature streams for cuts at and around every unit boundary
    SMALL      twelve units, for packets of a few bytes
    LAYOUTS    the 44.1 kHz family and the 1-, 3-, 5- and 6-channel (0x14) assignments
    DAMAGE     fixed, handled damage at chosen units

A fixture is a Case: bytes, channels, frames per standard unit, expected PCM frames, the unit that triggers the
fall-back (or None).  Packetisations are lists of cut positions (where each packet ends).
"""
import collections
import os
import re

import numpy as np

from tests.stream_tools import cuts_at_units, frame_offsets, major_syncs, padded_unit, splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = collections.namedtuple("Case", "data nch rpa frames trigger S cfg")

BASE_FEATS = ("CHAINED", "FIRRAND", "PARAMBLOCKS")
RICH_FEATS = BASE_FEATS + ("IIR", "MIDMATRIX", "MATRIXRAND", "QSS", "OUTSHIFT", "VARBLOCK", "MIXBOOKS", "MIDRESTART")

# name -> (substreams, rate code, seed)
BASES = {"s1r1": (1, 1, 7301), "s2r1": (2, 1, 7302), "s2r2": (2, 2, 7303),
         # 48 kHz: 40 frames per unit, and seeds (found by a scan on the oracle) where a lost FIR history in front of the
         # sync at unit 20 / 32 is still audible in the unit behind it -- see KEPT_HISTORY
         "fir_s1r0": (1, 0, 7425), "fir_s2r0": (2, 0, 7403)}
PAD_UNITS = (1, 4, 18, 21, 35)      # before any queue cut | itself the sync the queue begins at | mid-segment after four
                                    # cuts | mid-segment | the last unit
PAD_SIZE = 4200                     # > the 4 KB stage of k_coop
SPLICE_SYNC = 5                     # the tail begins at the sixth major sync = unit 20
# (seed 7317 would be next for S=2 / rate 1: its segment at unit 20 opens with FIR order 0 in every channel, so the history
#  in front of it changes nothing -- test_streaming_model.py would refuse it)
SPLICES = {"splice_s%dr%d" % (S, r): (S, r, 7360 if (S, r) == (2, 1) else 7310 + 3 * S + r) for S in (1, 2) for r in (0, 1, 2)}

# A predictor's memory is short: behind a restart a wrong FIR history has left the PCM after some tens of frames (9 to 61
# in the streams above), and a fall-back hands out nothing in front of the frames of the queue's first unit (that unit was
# decoded by the call that cut the queue at it).  So the history the tier keeps in `fir` reaches the PCM only where the
# trigger is the unit right behind a restarting sync and the wrong values live longer than that sync's own unit: these.
KEPT_HISTORY = ["fir_s1r0_pad21", "fir_s2r0_pad33"]

HANDOVER = ["%s_pad%d" % (b, w) for b in ("s1r1", "s2r1", "s2r2") for w in PAD_UNITS] + sorted(SPLICES) + KEPT_HISTORY

# name -> (substreams, rate code, SYNCONLY, seed)
BOUNDARY = {"rich_s1": (1, 1, False, 7321), "rich_s2": (2, 0, False, 7322),
            "rich_s1_synconly": (1, 2, True, 7323), "rich_s2_synconly": (2, 1, True, 7324)}

# name -> (assignment, rate code, seed)
SMALL = {"small_2ch_48k": (1, 0, 7331), "small_mono_44k": (0, 8, 7332)}

# name -> (assignment, rate code, substreams, seed)
LAYOUTS = {"rate8": (12, 8, 1, 7341), "rate9": (12, 9, 2, 7342), "rate10": (12, 10, 2, 7343),
           "asg0": (0, 1, 1, 7344), "asg2": (2, 0, 2, 7345), "asg6": (6, 2, 2, 7346), "asg0x14": (0x14, 9, 2, 7347)}

DAMAGE_BASES = ("recipe_2ss_40", "r2_6ch_60")
DAMAGE_KINDS = ("flip", "crc", "size")      # + "nosync", which has no unit of its own
DAMAGE_UNITS = (0, 1, 17, -1)

PACKET = 2011


def feats(syn, names):
    f = 0
    for n in names:
        f |= syn.SF[n]
    return f


def step_limits():
    """(units, bytes) one step of the stepping kernel takes: csrc/mlp_step.h"""
    h = open(os.path.join(ROOT, "libdvd-audio_amd", "csrc", "mlp_step.h")).read()
    return (int(re.search(r"#define DVDA_STEP_MAX_UNITS (\d+)u", h).group(1)),
            int(re.search(r"#define DVDA_STEP_MAX_BYTES (\d+)u", h).group(1)))


def _made(syn, cfg, seed):
    data, frames = syn.stream(cfg, seed)
    return Case(data, syn.channels(cfg.assignment), syn.rows_per_au(cfg.rate_code), frames, None, cfg.n_substreams, cfg)


def _base_cfg(syn, S, rate, n_aus=36, assignment=12, extra=()):
    return syn.make_cfg(assignment=assignment, rate_code=rate, n_substreams=S, n_aus=n_aus, profile=1,
                        features=feats(syn, BASE_FEATS + tuple(extra)), restart_interval=4)


_cache = {}


def case(syn, name):
    """the fixture `name` (made once per process)"""
    if name not in _cache:
        _cache[name] = _make(syn, name)
    return _cache[name]


def _make(syn, name):
    if name in BASES:
        S, rate, seed = BASES[name]
        return _made(syn, _base_cfg(syn, S, rate), seed)
    m = re.match(r"(\w+)_pad(\d+)$", name)
    if m:
        base, which = case(syn, m.group(1)), int(m.group(2))
        return base._replace(data=padded_unit(base.data, which, PAD_SIZE), trigger=which)
    m = re.match(r"(\w+)_(std|var)$", name)
    if m:                               # the two streams a splice is made of
        S, rate, seed = SPLICES[m.group(1)]
        return _made(syn, _base_cfg(syn, S, rate, extra=("VARROWS",) if m.group(2) == "var" else ()), seed)
    if name in SPLICES:
        std, var = case(syn, name + "_std"), case(syn, name + "_var")
        data = splice(std.data, var.data, SPLICE_SYNC)
        trigger = frame_offsets(data).index(major_syncs(data)[SPLICE_SYNC])
        # frames: the standard units in front and the tail's own, which only a decode of `var` counts
        # (test_streaming_model.py does)
        return std._replace(data=data, frames=None, trigger=trigger)
    if name in BOUNDARY:
        S, rate, synconly, seed = BOUNDARY[name]
        cfg = syn.make_cfg(assignment=12, rate_code=rate, n_substreams=S, n_aus=36, profile=1,
                           features=feats(syn, RICH_FEATS + (("SYNCONLY",) if synconly else ())), restart_interval=4)
        return _made(syn, cfg, seed)
    if name in SMALL:
        asg, rate, seed = SMALL[name]
        return _made(syn, _base_cfg(syn, 1, rate, n_aus=12, assignment=asg), seed)
    if name in LAYOUTS:
        asg, rate, S, seed = LAYOUTS[name]
        return _made(syn, _base_cfg(syn, S, rate, assignment=asg), seed)
    if name == "recipe_2ss_40":         # the stream of test_streaming_tier_mirrors_mlp_h[recipe]
        return _made(syn, syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=40), 77)
    if name == "r2_6ch_60":             # more than 48 units and more than 48 KB: one call with all of it is several steps
        return _made(syn, _base_cfg(syn, 1, 2, n_aus=60), 7351)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- framing
def unit_bounds(data):
    """[start of unit 0, start of unit 1, ..., end of the last complete unit]"""
    offs = frame_offsets(data)
    if not offs:
        return [0]
    last = offs[-1]
    return offs + [last + 2 * (((int(data[last]) & 0xF) << 8) | int(data[last + 1]))]


def unit_restarts(data, pos, S):
    """does every substream of the sync unit at `pos` open with a restart header?  (mlp_stream.c unit_restarts, restated)"""
    p, end0 = pos + 4 + 28, 0
    for s in range(S):
        e = (int(data[p]) << 8) | int(data[p + 1])
        if s == 0:
            end0 = (e & 0xFFF) * 2
        p += 4 if e & 0x8000 else 2
    if (int(data[p]) & 0xC0) != 0xC0:
        return False
    return S == 1 or (int(data[p + end0]) & 0xC0) == 0xC0


def restarting_syncs(data, S):
    """unit indices of the major syncs whose substreams all restart: where the tier cuts its queue"""
    offs = frame_offsets(data)
    syncs = set(major_syncs(data))
    return [i for i, o in enumerate(offs) if o in syncs and unit_restarts(data, o, S)]


# ---------------------------------------------------------------------------------------------- packetisations
def cuts_fixed(data, n):
    return list(range(n, len(data), n)) + [len(data)]


def cuts_whole(data):
    return [len(data)]


def cuts_around_units(data):
    """one byte before and one byte after every unit boundary"""
    inner = frame_offsets(data)[1:]
    return sorted({o - 1 for o in inner} | {o + 1 for o in inner}) + [len(data)]


def cuts_tiny(data, n):
    """n bytes at a time, with an empty packet after every tenth call"""
    out = []
    for i, c in enumerate(cuts_fixed(data, n)):
        out.append(c)
        if i % 10 == 9:
            out.append(c)
    return out


PACKETISATIONS = {"p2011": lambda d: cuts_fixed(d, PACKET), "units": cuts_at_units, "whole": cuts_whole}


def call_completing(cuts, end):
    """index of the first call after which the byte at end - 1 has been fed"""
    return next(i for i, c in enumerate(cuts) if c >= end)


def packets(data, cuts):
    lo = 0
    for hi in cuts:
        yield np.ascontiguousarray(data[lo:hi])
        lo = hi


class OracleDecoder:
    """mlp_oracle_open / decode_packet / close (oracle/mlp_oracle.h): the reference's mlp.h, packet by packet"""

    def __init__(self, oracle, nch):
        import ctypes
        L = self.lib = oracle.lib
        L.mlp_oracle_open.restype = ctypes.c_void_p
        L.mlp_oracle_open.argtypes = [ctypes.c_uint]
        L.mlp_oracle_decode_packet.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        L.mlp_oracle_decode_packet.restype = ctypes.c_uint
        L.mlp_oracle_close.argtypes = [ctypes.c_void_p]
        L.mlp_oracle_status.argtypes = [ctypes.c_void_p]
        L.mlp_oracle_status.restype = ctypes.c_uint
        L.mlp_oracle_channel_len.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        L.mlp_oracle_channel_len.restype = ctypes.c_size_t
        L.mlp_oracle_channel.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        L.mlp_oracle_channel.restype = ctypes.POINTER(ctypes.c_int32)
        self.nch = nch
        self.h = L.mlp_oracle_open(nch)
        assert self.h

    def decode_packet(self, piece):
        return int(self.lib.mlp_oracle_decode_packet(self.h, piece.ctypes.data if len(piece) else None, len(piece)))

    @property
    def status(self):
        return int(self.lib.mlp_oracle_status(self.h))

    def pcm(self):
        """[channels, frames]; None where the channels are of different lengths (the oracle goes on behind a unit that
        fails in its second substream, as the reference would if it did not assert)"""
        n = [int(self.lib.mlp_oracle_channel_len(self.h, c)) for c in range(self.nch)]
        if len(set(n)) != 1:
            assert self.status
            return None
        out = np.zeros((self.nch, n[0]), np.int32)
        for c in range(self.nch):
            if n[0]:
                out[c] = np.ctypeslib.as_array(self.lib.mlp_oracle_channel(self.h, c), shape=(n[0],))
        return out

    def close(self):
        if self.h:
            self.lib.mlp_oracle_close(self.h)
            self.h = None


def oracle_calls(oracle, nch, data, cuts):
    """-> (every call's return, PCM [nch, frames], status) of the oracle fed `data` cut at `cuts`"""
    od = OracleDecoder(oracle, nch)
    try:
        rets = [od.decode_packet(p) for p in packets(data, cuts)]
        return rets, od.pcm(), od.status
    finally:
        od.close()


# ---------------------------------------------------------------------------------------------- damage
def damaged(data, kind, k):
    """-> (copy of `data` with damage `kind` at unit k (negative: from the end), k as a unit index of the result)
    flip: a payload bit of the unit; crc: the unit's last byte, the last substream's CRC-8, inverted; size: the unit's
    size field set to one word; nosync: the first unit removed (k ignored, 0 returned)"""
    b = unit_bounds(data)
    n = len(b) - 1
    k = k % n
    out = data.copy()
    if kind == "flip":
        out[(b[k] + b[k + 1]) // 2] ^= 0x04
    elif kind == "crc":
        out[b[k + 1] - 1] ^= 0xFF
    elif kind == "size":
        out[b[k]] = int(out[b[k]]) & 0xF0
        out[b[k] + 1] = 1
    elif kind == "nosync":
        return data[b[1]:].copy(), 0
    else:
        raise KeyError(kind)
    return out, k


def steps_of_call(bounds, first_unit, end_unit):
    """how mlp_stream.c deals the units [first_unit, end_unit) of one call to steps: greedily, up to step_limits() each
    -> [(first, end), ...]"""
    max_units, max_bytes = step_limits()
    out, at = [], first_unit
    while at < end_unit:
        e = at
        while e < end_unit and e - at < max_units and bounds[e + 1] - bounds[at] <= max_bytes:
            e += 1
        assert e > at
        out.append((at, e))
        at = e
    return out


def handed_out_before_failure(bounds, cuts, k):
    """(units handed out when the stepping path fails at unit k, units completed by the calls in front of the failing
    one): the failing step's units are not handed out, the steps of the same call in front of it are
    (mlp_stream.c: the `failed` branch)"""
    i = call_completing(cuts, bounds[k + 1])
    before = 0 if i == 0 else max(u for u in range(len(bounds)) if bounds[u] <= cuts[i - 1])
    end_unit = max(u for u in range(len(bounds)) if bounds[u] <= cuts[i])
    for first, end in steps_of_call(bounds, before, end_unit):
        if first <= k < end:
            return first, before
    raise AssertionError("unit %d is not in call %d" % (k, i))
