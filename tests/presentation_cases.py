"""The presentation strip's cases (csrc/mlp_present.h: k_pp_streams, k_pp_size, k_pp_len, k_pp_fill, k_pp_copy and its
pp_unit / pp_copy; csrc/mlp_present_run.h: present_index and the getters), one table for the CPU file
(tests/test_presentation_cases_model.py: the premises, on the model's own walk of the bytes) and the GPU file
(tests/test_gpu_presentation_edges.py: the presentation buffer read back with dvda_mlp_hip_present_read, byte for byte).

TEST INFRASTRUCTURE.  Plain Python, no GPU.  A case is a Batch: source streams, where they lie in the flat buffer, and
what of them is decoded.  Every expected value comes from tests/presentation_model.py (strip / expect) and, for
framing, from tests/index_model.py run over the model's presentation buffer.

Two kinds of stream:
  decodable   rearranged REAL generator units (stream_tools, index_model's builders): indexed, decoded, held to the model
  hand-made   a real first unit (so that k is found) and behind it well-framed units whose directory words and sizes are
              chosen and whose bodies are pseudo-random bytes: groups "sweep", "clamps" and "geometry".  They give the
              source index what it looks at in a unit (index_model: the size field, the major-sync pattern, the
              substream count and the five parameters of the stream's own sync) and are ONLY indexed: no decode, no
              oracle and no reference ever sees them (Batch.decode is None, and the CPU file asserts it).

Where a stream lies: the batch tier takes 16-byte aligned stream starts only (a misaligned range is refused,
include/dvda_mlp_hip.h), so phase 0 is every start phase it accepts.  The phases of the copies are moved INSIDE the
streams, as tests/test_gpu_index.py does for major syncs: by the sizes of the units in front (hand-made streams: an
"adjuster" unit in front of every target unit; generator streams: stream_tools.padded_unit).

The body classes of pp_copy, with h = (16 - dst) & 15 the halfword head, n the body's bytes (even) and
chunks = (n - h) >> 4 the 16-byte stores:
    1  n = 0                      2  0 < n < h                  3  n = h (h > 0)
    4  h < n < h + 16             5  chunks in 1 .. 63          6a chunks = 64, tail 0     6b chunks = 64, tail > 0
    7  chunks = 65                8  chunks >= 129              9  the largest body of a unit of 8 190 bytes (8 182)
Class 2 needs an even n with 0 < n < h, so h >= 4: it exists at the dst phases 2 .. 12 (and not at 0 and 14), at
every src - dst phase; class 3 needs h > 0.  The coverage the CPU file asserts is "wherever the class exists".
"""
import collections

import numpy as np

from tests import index_model as im
from tests import presentation_model as pm
from tests import stream_tools
from tests.conceal_cases import fix_checks, substream_starts

MAX_UNIT = 8190
MAX_BODY = MAX_UNIT - 4 - 2 - 2        # plain unit, one directory word per substream, nothing in substream 1

# decode: None (bytes and index only) or a dict: nch (channel count of a one-substream source, per stream, or None),
# kinds (per stream: "good", "none", "envelope", "cut"); where the stripped streams go to the compiled reference too: rate
# (their rate code) and names (per stream, for the digests' keys)
Batch = collections.namedtuple("Batch", "name group streams starts decode note")


# ------------------------------------------------------------------------------------------------ the model of a batch

def present_bytes(stream):
    """the presentation stream of one source stream as the strip kernels hand it to the second index: a stream that
    does not begin with a major sync has none; a one-substream stream is its complete access units; a two-substream
    stream is presentation_model.strip of it (empty when there is no k)"""
    D = np.asarray(stream, np.uint8)
    S = pm.substreams_of(D)
    if S == 0:
        return np.zeros(0, np.uint8)
    if S == 1:
        return D[:pm.consumed(D)].copy()
    return pm.strip(D)[0]


_BUFFER = {}


def present_buffer(batch):
    """-> (buf: bound + 64 bytes, offs, lens, bound) of the batch: every stream at the running sum of the lengths in
    front of it, each rounded up to 16; zeros everywhere else; bound = what the second index is told to scan (cached)"""
    if batch.name not in _BUFFER:
        flat, offs, lens, total = source(batch)
        n = len(batch.streams)
        bound = ((total + 15) & ~15) + 16 * n
        buf = np.zeros(bound + 64, np.uint8)
        poffs, plens, pos = [], [], 0
        cache = {}
        for s in batch.streams:
            key = id(s)
            if key not in cache:
                cache[key] = present_bytes(s)
            p = cache[key]
            poffs.append(pos)
            plens.append(len(p))
            buf[pos:pos + len(p)] = p
            pos += (len(p) + 15) & ~15
        buf.setflags(write=False)
        _BUFFER[batch.name] = (buf, poffs, plens, bound)
    return _BUFFER[batch.name]


def source(batch):
    """-> (flat with 64 spare bytes, offs, lens, total) of the batch's source streams"""
    return im.lay_out(batch.streams, batch.starts)


_INNER = {}


def inner_index(batch):
    """what the second index has to find: index_model.expect over the model's presentation buffer (cached)"""
    if batch.name not in _INNER:
        buf, offs, lens, bound = present_buffer(batch)
        _INNER[batch.name] = im.expect(buf, bound, np.asarray(offs, np.uint64), np.asarray(lens, np.uint64))
    return _INNER[batch.name]


# ------------------------------------------------------------------------------------------------ the walk

Rec = collections.namedtuple("Rec", "stream unit sync dir0 dir1 n dst src clamped")


def walk(batch):
    """every access unit of every two-substream stream of the batch that has a presentation, as pp_copy meets its body:
    n bytes from absolute source offset src to absolute offset dst of the presentation buffer (presentation_model's
    _unit_parts, the batch's layout).  clamped: a range of the unit was cut to the unit."""
    _, soffs, _, _ = source(batch)
    _, poffs, plens, _ = present_buffer(batch)
    out = []
    for i, s in enumerate(batch.streams):
        D = np.asarray(s, np.uint8)
        if pm.substreams_of(D) != 2 or not plens[i]:
            continue
        dpos = poffs[i]
        for j, p in enumerate(stream_tools.frame_offsets(D)):
            fe = p + im.unit_size(D, p)
            sync, (d, d_end), (q, q_end) = pm._unit_parts(D, p, fe, 2)
            dpos += 4 + sync + (d_end - d)
            out.append(Rec(i, j, sync, d_end - d, q - d_end, q_end - q, dpos, int(soffs[i]) + q,
                           _clamps(D, fe, d, d_end, q, q_end)))
            dpos += q_end - q
    return out


def _clamps(D, fe, d, d_end, q, q_end):
    """which ranges of the unit that ends at fe were cut to it: "no_dir" (it ends before substream 0's word), "dir0" (inside
    substream 0's words), "no_dir1" (before substream 1's word), "dir1" (inside substream 1's words), "end0" (substream 0's
    bytes leave the unit)"""
    if d + 2 > fe:
        return frozenset(["no_dir"])
    out = set()
    w0 = (int(D[d]) << 8) | int(D[d + 1])
    if (4 if w0 & 0x8000 else 2) != d_end - d:
        out.add("dir0")
    if d_end + 2 > fe:
        out.add("no_dir1")
    elif (4 if int(D[d_end]) & 0x80 else 2) != q - d_end:
        out.add("dir1")
    if (w0 & 0xFFF) * 2 != q_end - q:
        out.add("end0")
    return frozenset(out)


def body_class(n, dst):
    h = (16 - dst) & 15
    if n == 0:
        return "1"
    if n < h:
        return "2"
    if n == h:
        return "3"
    chunks, tail = (n - h) >> 4, (n - h) & 15
    if chunks == 0:
        return "4"
    if chunks < 64:
        return "5"
    if chunks == 64:
        return "6b" if tail else "6a"
    if chunks == 65:
        return "7"
    return "8" if chunks >= 129 else "mid"


def pair(rec):
    """(dst phase of the body, src - dst phase), both mod 16"""
    return rec.dst % 16, (rec.src - rec.dst) % 16


def exists(cls, d):
    """is there a body of class cls at dst phase d?"""
    h = (16 - d) & 15
    return h >= 4 if cls == "2" else h > 0 if cls == "3" else True


# ------------------------------------------------------------------------------------------------ generator streams

_GEN = {}


def gen(syn, feat=0, seed=0, assignment=12, ss0=2, S=2, n_aus=48, rate=1, interval=8):
    """a generator stream (cached, read-only) -> bytes; feat: feature names joined by "|" (CHAINED brings FIRRAND, as
    tests/test_presentation_model.make_stream has it)"""
    key = (feat, seed, assignment, ss0, S, n_aus, rate, interval)
    if key not in _GEN:
        f = 0
        for name in (feat.split("|") if feat else []):
            f |= syn.SF[name] | (syn.SF["FIRRAND"] if name == "CHAINED" else 0)
        kw = dict(ss0_channels=ss0) if S == 2 else {}
        cfg = syn.make_cfg(assignment=assignment, rate_code=rate, n_substreams=S, n_aus=n_aus, profile=1 if f else 0,
                           features=f, restart_interval=interval, **kw)
        b = syn.stream(cfg, 9000 + 13 * seed)[0]
        b.setflags(write=False)
        _GEN[key] = b
    return _GEN[key]


def first_unit(syn):
    """the first access unit of a two-substream generator stream (assignment 12, k = 2): what opens every hand-made stream"""
    b = gen(syn, 0, 1, n_aus=2)
    return b[:stream_tools.frame_offsets(b)[1]]


# ------------------------------------------------------------------------------------------------ hand-made units

def unit(rng, u0, n0, n1, x0=False, x1=False, sync=False, w0=None, w1=None, size=None):
    """a two-substream access unit: substream 0 of n0 bytes and substream 1 of n1 bytes of pseudo-random bytes behind
    their directory words (x0 / x1: with an extra word), behind the 28 bytes of u0's major sync when `sync`.  w0 / w1
    override the directory words' values, size the unit's size: the clamp cases, cut to `size` bytes."""
    w0 = ((0x8000 if x0 else 0) | (n0 // 2)) if w0 is None else w0
    w1 = ((0x8000 if x1 else 0) | ((n0 + n1) // 2)) if w1 is None else w1
    assert n0 % 2 == 0 and n1 % 2 == 0 and (n0 + n1) // 2 <= 0xFFF
    parts = [np.array([w0 >> 8, w0 & 0xFF], np.uint8)]
    if w0 & 0x8000:
        parts.append(rng.randint(0, 256, 2).astype(np.uint8))
    parts.append(np.array([w1 >> 8, w1 & 0xFF], np.uint8))
    if w1 & 0x8000:
        parts.append(rng.randint(0, 256, 2).astype(np.uint8))
    parts.append(rng.randint(0, 256, n0 + n1).astype(np.uint8))
    rest = np.concatenate(parts)
    full = 4 + (28 if sync else 0) + len(rest)
    size = full if size is None else size
    assert size % 2 == 0 and 4 <= size <= MAX_UNIT and size <= full
    hdr = np.array([(int(rng.randint(0, 16)) << 4) | ((size // 2) >> 8), (size // 2) & 0xFF,
                    int(rng.randint(0, 256)), int(rng.randint(0, 256))], np.uint8)
    return np.concatenate([hdr, u0[4:32] if sync else np.zeros(0, np.uint8), rest])[:size]


COMBOS = [(x0, x1, sync) for sync in (False, True) for x0 in (False, True) for x1 in (False, True)]


def steered(rng, u0, pos, d, e, n, x0, x1, sync):
    """-> [adjuster unit, target unit]: the target's body of n bytes goes to dst phase d from src phase d + e, after
    `pos` = (source bytes, presentation bytes) of the stream so far.  The adjuster is a plain unit with a bytes of
    substream 0 (6 + a presentation bytes) and s bytes of substream 1 (8 + a + s source bytes)."""
    src, dst = pos
    over_d = 4 + (28 if sync else 0) + (4 if x0 else 2)
    over_s = over_d + (4 if x1 else 2)
    a = (d - over_d - dst - 6) % 16
    s = (d + e - over_s - src - 8 - a) % 16
    n1 = min(MAX_UNIT - over_s - n, int(rng.randint(0, 4)) * 2)        # a few bytes of substream 1 where the unit has room
    return [unit(rng, u0, a, s), unit(rng, u0, n, n1, x0, x1, sync)]


def body_len(cls, d, rng, turn):
    h = (16 - d) & 15
    even = lambda lo, hi: lo + 2 * int(rng.randint(0, (hi - lo) // 2 + 1))       # even value in [lo, hi]
    if cls == "1":
        return 0
    if cls == "2":
        return even(2, h - 2)
    if cls == "3":
        return h
    if cls == "4":
        return h + even(2, 14)
    if cls == "5":
        return h + 16 * (1, 2, 7, 31, 62, 63)[turn % 6] + even(0, 14)
    if cls == "6a":
        return h + 1024
    if cls == "6b":
        return h + 1024 + even(2, 14)
    if cls == "7":
        return h + 16 * 65 + even(0, 14)
    if cls == "8":
        return h + 16 * (129, 130, 193, 257)[turn % 4] + even(0, 14)
    assert cls == "9"
    return MAX_BODY


def sweep_stream(syn, seed, classes, pairs):
    """a real first unit, then for every (class, d, e) of classes x pairs where the class exists an adjuster and the
    target; the directory shapes and sync / plain turn with the targets"""
    rng = np.random.RandomState(seed)
    u0 = first_unit(syn)
    parts = [u0]
    src, dst = len(u0), len(pm.strip(u0)[0])
    turn = 0
    for cls in classes:
        for d, e in pairs:
            if not exists(cls, d):
                continue
            x0, x1, sync = (False, False, False) if cls == "9" else COMBOS[(turn + turn // 8) % 8]
            n = body_len(cls, d, rng, turn)
            for u in steered(rng, u0, (src, dst), d, e, n, x0, x1, sync):
                parts.append(u)
                src += len(u)
                dst += _out_len(u)
            turn += 1
    b = np.concatenate(parts)
    b.setflags(write=False)
    return b


def _out_len(u):
    """presentation bytes of one well-framed hand-made unit"""
    sync, (d, d_end), (q, q_end) = pm._unit_parts(u, 0, len(u), 2)
    return 4 + sync + (d_end - d) + (q_end - q)


ALL_PAIRS = [(d, e) for d in range(0, 16, 2) for e in range(0, 16, 2)]
# the eight src - dst phases, each at another dst phase with h > 0
EIGHT = [((2 + 6 * k) % 16 or 8, 2 * k) for k in range(8)]


def build_sweep(syn):
    streams = [sweep_stream(syn, 101, ["2"], ALL_PAIRS), sweep_stream(syn, 102, ["4"], ALL_PAIRS),
               sweep_stream(syn, 103, ["5"], ALL_PAIRS), sweep_stream(syn, 104, ["7"], ALL_PAIRS),
               sweep_stream(syn, 105, ["1", "3", "6a", "6b", "8", "9"], EIGHT)]
    return [Batch("sweep", "sweep", streams, None, None, "hand-made: only indexed")]


def build_clamps(syn):
    """behind a good first unit: units that end before or inside their directory, directory words that promise more
    than the unit holds, and good hand-made units between them so that a wrong size shifts what follows"""
    rng = np.random.RandomState(201)
    u0 = first_unit(syn)
    good = lambda: unit(rng, u0, 2 * int(rng.randint(3, 40)), 2 * int(rng.randint(0, 20)))
    parts = [u0]
    # plain units of 4, 6, 8 and 10 bytes; the directory words say 40 and 60 words
    for size in (4, 6, 8, 10):
        parts += [unit(rng, u0, 40, 40, w0=20, w1=40, size=size), good()]
    # the same with extra-word flags: at 6 bytes substream 0's flagged word is the unit's last two bytes, at 8 bytes its
    # extra word is (and substream 1 has no word), at 10 substream 1's flagged word is
    for size in (6, 8, 10):
        parts += [unit(rng, u0, 40, 40, w0=0x8000 | 20, w1=0x8000 | 40, size=size), good()]
    parts += [unit(rng, u0, 40, 40, w0=20, w1=0x8000 | 40, size=8), good()]
    # sync units of 32, 34, 36 and 38 bytes, with and without the flags
    for size in (32, 34, 36, 38):
        parts += [unit(rng, u0, 40, 40, sync=True, w0=20, w1=40, size=size), good()]
        parts += [unit(rng, u0, 40, 40, sync=True, w0=0x8000 | 20, w1=0x8000 | 40, size=size), good()]
    # substream_end_0 larger than what is left of the unit: by one word, by a lot, and the field's maximum
    parts += [unit(rng, u0, 60, 0, w0=31, w1=31), good(), unit(rng, u0, 60, 20, w0=2000, w1=2000, sync=True), good(),
              unit(rng, u0, 0, 0, w0=0xFFF, w1=0xFFF), good()]
    # substream_end_1 < substream_end_0
    parts += [unit(rng, u0, 40, 20, w0=20, w1=10), good(), unit(rng, u0, 40, 20, w0=20, w1=0, sync=True), good()]
    b = np.concatenate(parts)
    b.setflags(write=False)
    return [Batch("clamps", "clamps", [b, np.concatenate([u0, good()]), b], None, None, "hand-made: only indexed")]


def build_geometry(syn):
    """single-unit two-substream streams of 42 bytes, the shortest unit that still gives k (a major sync, two directory
    words, six bytes of substream 0: the restart header's bits 40-43); the input timing counts the streams"""
    u0 = first_unit(syn)
    q, ends, _ = substream_starts(u0, 0, 2)
    assert ends[0] >= 6
    base = np.concatenate([u0[:32], np.array([0, 3, 0, 3], np.uint8), u0[q:q + 6]])
    base[0], base[1] = int(u0[0]) & 0xF0, 21
    out = []
    made = {}
    for n in (255, 256, 257, 1025, 16385):
        streams = []
        for i in range(n):
            if i not in made:
                s = base.copy()
                s[2], s[3] = i >> 8, i & 0xFF
                s.setflags(write=False)
                made[i] = s
            streams.append(made[i])
        out.append(Batch("geometry%d" % n, "geometry", streams, [48 * i for i in range(n)], None,
                         "hand-made: only indexed"))
    return out


# ------------------------------------------------------------------------------------------------ decodable cases

def build_large(syn):
    """rate code 2, five channels in substream 0: bodies of one to two and a half KB -- the lane loop's second and third
    turn on streams that decode"""
    streams, names = [], []
    for asg in (12, 20):
        for feat in (0, "CHAINED", "FULLSCALE", "FULLSCALE|CHAINED"):
            streams.append(gen(syn, feat, 3, asg, 5, 2, 12, 2))
            names.append("%d_%s" % (asg, feat or "plain"))
    return [Batch("large", "large", streams, None, dict(nch=[None] * 8, rate=2, kinds=["good"] * 8, names=names), "")]


def phased_segments(b):
    """`b` with its major syncs 1 .. 8 moved to the phases 2, 4, .., 14, 0 of a 16-byte chunk (zero bytes behind the last
    substream of the unit in front of each, stream_tools.padded_unit)"""
    out = b
    for k in range(1, 9):
        at = stream_tools.major_syncs(out)[k]
        out = im.place_sync(out, 0, k, at + ((2 * k - at) % 16 or 16))
    assert [p % 16 for p in stream_tools.major_syncs(out)[:9]] == [0, 2, 4, 6, 8, 10, 12, 14, 0]
    return out


def build_one_substream(syn):
    """one-substream streams under the mode (the k == 0 path of k_pp_copy: one pp_copy per source segment): nine
    segments of two units at 192 kHz, their starts at all eight phases; 2-channel 48 kHz beside them"""
    six = phased_segments(gen(syn, "CHAINED", 4, 12, S=1, n_aus=18, rate=2, interval=2))
    two = phased_segments(gen(syn, 0, 5, 1, S=1, n_aus=18, rate=0, interval=2))
    plain = gen(syn, 0, 6, 12, S=1, n_aus=18, rate=2, interval=2)
    return [Batch("one_substream", "one", [six, two, plain, six], None,
                  dict(nch=[6, 2, 6, 6], kinds=["good"] * 4), "one substream: the stream itself, byte for byte")]


def cut_in_last_unit(b, keep):
    """the stream cut `keep` bytes into its last access unit"""
    return np.ascontiguousarray(b[:stream_tools.frame_offsets(b)[-1] + keep])


def build_mixed(syn):
    rng = np.random.RandomState(301)
    goods = [gen(syn, "CHAINED", 0, n_aus=9), gen(syn, 0, 1, 20, 3, n_aus=9), gen(syn, 0, 2, 1, S=1, n_aus=9, rate=0),
             gen(syn, "DISC|CHAINED", 3, 12, 5, n_aus=9), gen(syn, 0, 4, 6, 1, n_aus=9), gen(syn, "CHAINED", 5, 12, S=1, n_aus=9)]
    good_nch = [None, None, 2, None, None, 6]
    garbage = rng.randint(0, 256, 600).astype(np.uint8)
    garbage[4:8] = 0
    assert not len(im.candidates(np.concatenate([garbage, np.zeros(64, np.uint8)]), len(garbage)))
    two = gen(syn, 0, 7, n_aus=9)                     # nine units, restart interval 8: the last one is a major sync
    last = stream_tools.frame_offsets(two)[-1]
    assert stream_tools.is_major_sync(two, last)
    q, ends, _ = substream_starts(two, 0, 2)
    no_header = two.copy()
    assert int(no_header[q]) & 0xC0 == 0xC0
    no_header[q] &= 0x7F
    six = two.copy()
    six[q + 5] = (int(six[q + 5]) & 0x0F) | 0x50
    lq, lends, _ = substream_starts(two, last, 2)
    bad = [("none", garbage), ("none", np.zeros(0, np.uint8)), ("envelope", no_header), ("envelope", six),
           ("cut", cut_in_last_unit(two, 2)), ("cut", cut_in_last_unit(two, 20)), ("cut", cut_in_last_unit(two, 34)),
           ("cut", cut_in_last_unit(two, lq - last + lends[0] // 2))]
    streams, kinds, nch = [], [], []
    for i, (kind, b) in enumerate(bad):
        g = i % len(goods)
        streams += [goods[g], b]
        kinds += ["good", kind]
        nch += [good_nch[g], None]
    streams.append(goods[2])
    kinds.append("good")
    nch.append(good_nch[2])
    return [Batch("mixed", "mixed", streams, None, dict(nch=nch, kinds=kinds),
                  "A source stream the index could not frame (DVDA_ST_NO_SYNC, _IRREGULAR, _CAPACITY) keeps that status "
                  "and decodes nothing; a first unit whose substream 0 opens with no restart header, or a k above 5: "
                  "DVDA_ST_ENVELOPE, nothing decoded")]


def false_syncs_in_substream_1(b, unit, n):
    """index_model.with_false_syncs, and substream 1's end moved behind the new bytes: they are substream 1's (its check
    bytes no longer hold: the full decode's business)"""
    out = im.with_false_syncs(b, unit, n, None, 0x11, 40)
    p = stream_tools.frame_offsets(out)[unit]
    q = p + (32 if stream_tools.is_major_sync(out, p) else 4)
    w0 = (int(out[q]) << 8) | int(out[q + 1])
    q1 = q + (4 if w0 & 0x8000 else 2)
    w1 = (int(out[q1]) << 8) | int(out[q1 + 1])
    w1 = (w1 & 0xF000) | ((w1 & 0xFFF) + n * 20)
    out[q1], out[q1 + 1] = w1 >> 8, w1 & 0xFF
    return out


def false_syncs_in_substream_0(b, unit, n):
    """n headers of a major-sync access unit with the stream's own parameters, 40 bytes apart, in front of the check
    bytes of substream 0 of access unit `unit` (behind the last block: read by nobody, covered by parity and CRC-8, which
    are written again) -- so they are substream 0's bytes, and the stream decodes as before"""
    b = np.asarray(b, np.uint8)
    p = stream_tools.frame_offsets(b)[unit]
    q, ends, check = substream_starts(b, p, 2)
    assert check
    at = q + ends[0] - 2
    tail = np.zeros(40 * n, np.uint8)
    f = im.fake_sync(im.sync_params(b, 0), 2, 0x11)
    for k in range(n):
        tail[40 * k:40 * k + 32] = f
    out = np.concatenate([b[:at], tail, b[at:]])
    size = im.unit_size(b, p) + len(tail)
    assert size <= MAX_UNIT
    out[p], out[p + 1] = (int(b[p]) & 0xF0) | ((size // 2) >> 8), (size // 2) & 0xFF
    d = p + (32 if stream_tools.is_major_sync(b, p) else 4)
    for _ in range(2):
        w = (int(out[d]) << 8) | int(out[d + 1])
        w2 = (w & 0xF000) | ((w & 0xFFF) + len(tail) // 2)
        out[d], out[d + 1] = w2 >> 8, w2 & 0xFF
        d += 4 if w & 0x8000 else 2
    fix_checks(out, p, 2)
    return out


# (name, what the model must make of it: (PCM frames, oracle status) of the presentation, of the full decode)
SYNC_CLAIMS = collections.OrderedDict(
    false_in_ss1=((1920, 0), None), false_in_ss0=((1920, 0), (1920, 0)), assignment_changed=((1920, 0), (1840, 2)),
    g1_bps_changed=((1840, 2), (1840, 2)), synconly=((1920, 0), (1920, 0)))


def build_sync(syn):
    b = gen(syn, 0, 8, n_aus=24)                # 24 units of 80 frames, major syncs at 0, 8 and 16
    assert len(stream_tools.major_syncs(b)) == 3
    streams = [false_syncs_in_substream_1(false_syncs_in_substream_1(b, 3, 5), 16, 3),
               false_syncs_in_substream_0(false_syncs_in_substream_0(b, 5, 3), 8, 2),
               stream_tools.change_sync_params(b, (1,), assignment=20)[0],
               stream_tools.change_sync_params(b, (1,), g1_bps=0)[0],
               gen(syn, "SYNCONLY|CHAINED", 9, n_aus=24)]
    for s in streams:
        s.setflags(write=False)
    note = ("major sync: its 28 bytes with the substream count set to 1 and the 5-bit channel assignment set to the "
            "identity assignment of k channels; PCM, status, pcm_frames, mlp_frames and segments are those of that "
            "stream: damage confined to substream 1's bytes does not touch the presentation")
    return [Batch("sync", "sync", streams, None,
                  dict(nch=[None] * 5, rate=1, kinds=["good"] * 5, names=list(SYNC_CLAIMS)), note)]


def build_reuse(syn):
    """the batches of the buffer-reuse sequences: the big one's presentation buffer reaches far behind the small one's"""
    big = [gen(syn, ("CHAINED", 0, "DISC|CHAINED")[i % 3], 20 + i, n_aus=24) for i in range(6)]
    small = [gen(syn, "CHAINED", 30, n_aus=8)]
    return [Batch("reuse_big", "reuse", big, None, dict(nch=[None] * 6, kinds=["good"] * 6), ""),
            Batch("reuse_small", "reuse", small, None, dict(nch=[None], kinds=["good"]), "")]


# sequences of (batch name, presentation mode) on one context; the last step is held to a fresh context
REUSE_SEQUENCES = collections.OrderedDict(
    big_small=[("reuse_big", 1), ("reuse_small", 1)],
    small_big=[("reuse_small", 1), ("reuse_big", 1)],
    big_full_small=[("reuse_big", 1), ("reuse_big", 0), ("reuse_small", 1)])

BUILDERS = collections.OrderedDict(sweep=build_sweep, clamps=build_clamps, geometry=build_geometry, large=build_large,
                                   one=build_one_substream, mixed=build_mixed, sync=build_sync, reuse=build_reuse)
HAND_MADE = ("sweep", "clamps", "geometry")
_BATCHES = {}


def batches(syn, group):
    """the group's batches, by name (cached: read-only)"""
    if group not in _BATCHES:
        _BATCHES[group] = collections.OrderedDict((b.name, b) for b in BUILDERS[group](syn))
    return _BATCHES[group]


def batch(syn, name):
    for group in BUILDERS:
        if name in NAMES[group]:
            return batches(syn, group)[name]
    raise KeyError(name)


NAMES = dict(sweep=["sweep"], clamps=["clamps"], geometry=["geometry%d" % n for n in (255, 256, 257, 1025, 16385)],
             large=["large"], one=["one_substream"], mixed=["mixed"], sync=["sync"], reuse=["reuse_big", "reuse_small"])


# ------------------------------------------------------------------------------------------------ expected records

def expected_info(batch, i, oracle):
    """-> (what dvda_mlp_hip_stream_info has to say of stream i of a decodable batch after the decode, as a dict; the
    model's PCM).  status: which of DVDA_ST_TRUNCATED | DVDA_ST_SYNC_CHANGE are set; no bit outside DVDA_ST_BENIGN may be
    (the informational bits the fast pass leaves are not the model's)"""
    assert batch.decode is not None, "a hand-made stream is only indexed"
    s = np.asarray(batch.streams[i], np.uint8)
    kind = batch.decode["kinds"][i]
    assert kind in ("good", "cut")
    x = inner_index(batch).streams[i]
    assert x.resolvable
    pcm, frames, ost, k = pm.expect(s, oracle, batch.decode["nch"][i])
    own = im.sync_params(s, 0)
    must = (im.TRUNCATED if kind == "cut" else 0) | (im.SYNC_CHANGE if ost & 2 else 0)
    assert ost & ~2 == 0 and x.status & ~im.SYNC_CHANGE == 0 and bool(x.status & im.SYNC_CHANGE) == bool(ost & 2)
    return dict(mlp_frames=x.mlp_frames, pcm_frames=frames, bytes_consumed=pm.consumed(s), channels=k,
                substreams=pm.substreams_of(s), assignment=own[4], group0_bps=own[0], group1_bps=own[1],
                group0_rate=own[2], group1_rate=own[3], segments=x.segments, status=must), pcm
