"""The frame index as the reference would see it, serially (plain Python / numpy; no GPU, no ctypes).

Not a restatement of csrc/mlp_index.h: the reference has no index.  It reads one access unit after the other by the
12-bit size field (src/mlp.c:384-405), takes a unit that begins with a major sync (src/mlp.c:614-654) of the stream's
parameters for a restart point and drops one whose major sync announces other parameters (src/mlp.c:449-460).  What
that serial walk finds, stream by stream, is what the GPU index has to report (include/dvda_mlp_hip.h): the live
segments, the access units that yield PCM, the bytes covered, the status bits -- and every OTHER place in the buffer
that passes the major-sync test is a candidate the index has to retire (DVDA_ST_FALSE_SYNC, no frames).

Two classes of stream (a condition of the input, asserted by the case builders, never a measurement):
  resolvable  the stream begins with a major sync, no false candidate's own size chain lands on another candidate, and
              at most MAX_DROP false candidates with the stream's own parameters sit inside one segment: the records
              of expect() are asserted exactly;
  the rest    the index may not be able to tell the chains apart: it has to say DVDA_ST_IRREGULAR and hand out no PCM
              under a clean status -- nothing more is asserted.

The case builders (below the model) rearrange REAL generator units with tests/stream_tools.py, so that the substream
checks and the decode stay meaningful: every benign case decodes, and is held to the oracle.
"""
import numpy as np

from tests import stream_tools

NO_SYNC, SYNC_CHANGE, PARITY, CRC, EOF, ENVELOPE = 1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 9
IRREGULAR, TRUNCATED, CAPACITY, FALSE_SYNC = 1 << 16, 1 << 21, 1 << 22, 1 << 24
INDEX_BITS = NO_SYNC | SYNC_CHANGE | EOF | ENVELOPE | IRREGULAR | TRUNCATED | CAPACITY | FALSE_SYNC
MAX_DROP = 64           # own-parameter false candidates inside one segment the index promises to resolve
ROWS_PER_AU = {0: 40, 8: 40, 1: 80, 9: 80, 2: 160, 10: 160}
WALK_CAP = 1 << 16      # steps of a false candidate's own walk the classifier follows (more: not resolvable)


# ------------------------------------------------------------------------------------------------ the model

def unit_size(flat, p):
    return 2 * (((int(flat[p]) & 0x0F) << 8) | int(flat[p + 1]))


def is_major_sync(flat, p, limit):
    """the major-sync test at even offset p of bytes that end at `limit`"""
    return (p + 32 <= limit and unit_size(flat, p) >= 32 and int(flat[p + 4]) == 0xF8 and int(flat[p + 5]) == 0x72 and
            int(flat[p + 6]) == 0x6F and int(flat[p + 7]) == 0xBB and (int(flat[p + 20]) >> 4) in (1, 2))


def sync_params(flat, p):
    """the five stream parameters dvda_params_equal compares: (g0 bps, g1 bps, g0 rate, g1 rate, assignment)"""
    return (int(flat[p + 8]) >> 4, int(flat[p + 8]) & 0xF, int(flat[p + 9]) >> 4, int(flat[p + 9]) & 0xF,
            int(flat[p + 11]) & 0x1F)


def candidates(flat, total):
    """every even absolute offset p that passes the major-sync test against the end of the buffer: brute force over
    all of them (as array operations: the tile-count case has 2^27 offsets)"""
    a = np.asarray(flat, np.uint8)[:total & ~1]
    if len(a) < 32:
        return np.zeros(0, np.int64)
    h = a.view("<u2")                                       # halfword k = bytes 2k, 2k + 1
    k = np.flatnonzero(h[2:-1] == 0x72F8)                   # bytes p + 4, p + 5 of p = 2k
    k = k[h[k + 3] == 0xBB6F]                               # bytes p + 6, p + 7
    p = 2 * k.astype(np.int64)
    p = p[p + 32 <= total]
    size = 2 * (((a[p].astype(np.int64) & 0x0F) << 8) | a[p + 1])
    count = a[p + 20] >> 4
    return p[(size >= 32) & ((count == 1) | (count == 2))]


def check_ranges(offs, lens, total):
    """The ranges as the index uses them -> (soff, slen, refused): the serial running maximum of the contract
    (include/dvda_mlp_hip.h, dvda_mlp_hip_index).  A range is refused, and gets length 0, if it is misaligned, leaves
    the buffer or starts before the end of ANY range in front of it.  A range that is misaligned or leaves the buffer
    has no end: it stands in nobody's way.  (One that is refused for its place alone still has an end, and a range
    behind it that starts before that end is refused too -- "the end of a stream in front of it", as the header has
    it; ascending ranges that merely repeat or go backwards never show the difference.)  A refused range is moved to
    the furthest end so far, so that the starts stay ascending."""
    soff, slen, refused, run = [], [], [], 0
    for o, l in zip(offs, lens):
        o, l = int(o), int(l)
        shaped = o % 16 == 0 and o <= total and l <= total - o
        ok = shaped and o >= run
        soff.append(min(o if ok else run, total))
        slen.append(l if ok else 0)
        refused.append(not ok)
        if shaped:
            run = max(run, o + l)
    return soff, slen, refused


class Seg:
    """a live segment: [off, end) holds nframes complete access units, ndrop of them dropped; flags: index bits"""

    def __init__(self, off):
        self.off, self.end, self.nframes, self.ndrop, self.flags = off, off, 0, 0, 0

    def record(self):
        return (self.off, self.end, self.nframes, self.flags)


class StreamExp:
    def __init__(self):
        self.resolvable = True
        self.refused = False
        self.capacity = False
        self.live = []
        self.mlp_frames = self.bytes_consumed = self.segments = self.status = 0
        self.sync = None            # dict of the first major sync's fields
        self.units = []             # absolute offsets of the complete access units (the true chain)


def walk_stream(flat, b, e):
    """the reference's serial framing of the bytes [b, e) that begin with a major sync -> StreamExp (without
    `segments` and the class: expect() adds them)"""
    x = StreamExp()
    own = sync_params(flat, b)
    x.sync = dict(group0_bps=own[0], group1_bps=own[1], group0_rate=own[2], group1_rate=own[3], assignment=own[4],
                  substreams=int(flat[b + 20]) >> 4)
    p, cur, tail = b, None, 0
    while True:
        # a major sync of the stream's own parameters opens a segment where it stands, whole, inside the range -- also
        # when the range ends inside its access unit (a segment of no units that says DVDA_ST_TRUNCATED)
        sync = is_major_sync(flat, p, e)
        if sync and sync_params(flat, p) == own:
            cur = Seg(p)
            x.live.append(cur)
        if p + 4 > e:
            tail = TRUNCATED if p != e else 0
            break
        size = unit_size(flat, p)
        if size < 4:
            tail = EOF
            break
        if p + size > e:
            tail = TRUNCATED
            break
        if sync and sync_params(flat, p) != own:        # a complete unit the reference reads and drops
            cur.ndrop += 1
            cur.flags |= SYNC_CHANGE
        x.units.append(p)
        cur.nframes += 1
        p += size
        cur.end = p
    x.live[-1].flags |= tail
    x.mlp_frames = sum(s.nframes - s.ndrop for s in x.live)
    x.bytes_consumed = p - b
    for s in x.live:
        x.status |= s.flags
    return x


def _own_walk_lands(flat, c, e, cand_set):
    """does the size chain that starts at false candidate c come down on another candidate?"""
    p = c
    for _ in range(WALK_CAP):
        if p + 4 > e:
            return False
        size = unit_size(flat, p)
        if size < 4 or p + size > e:
            return False
        p += size
        if p in cand_set:
            return True
    return True


class Index:
    """what expect() returns: cands (the kept candidate list = the segment indices), n_found, overflow, streams
    (StreamExp per caller's stream), and per kept candidate either its live Seg or None (retired)"""


def expect(flat, total, offs, lens, max_segments=None, cands=None):
    flat = np.asarray(flat, np.uint8)
    found = candidates(flat, total) if cands is None else cands
    ix = Index()
    ix.n_found = len(found)
    ix.overflow = max_segments is not None and len(found) > max_segments
    ix.cands = found[:max_segments] if ix.overflow else found
    soff, slen, refused = check_ranges(offs, lens, total)
    ix.soff, ix.slen = soff, slen
    n = len(soff)
    # the stream a candidate is looked up to: the last one that starts at or before it
    owner = np.searchsorted(np.asarray(soff, np.int64), ix.cands, "right") - 1
    cut = n
    if ix.overflow:
        cut = max(int(owner[-1]), 0) if len(owner) else 0
    ix.streams, ix.seg = [], [None] * len(ix.cands)
    cand_list = ix.cands.tolist()
    index_of = {c: i for i, c in enumerate(cand_list)}
    for s in range(n):
        b, e = soff[s], soff[s] + slen[s]
        mine = cand_list[np.searchsorted(owner, s, "left"):np.searchsorted(owner, s, "right")]
        if refused[s]:
            x = StreamExp()
            x.refused = True
            x.status = IRREGULAR | ENVELOPE
        elif s >= cut:
            x = StreamExp()
            x.capacity = True
        elif e - b < 32 or not is_major_sync(flat, b, e):
            x = StreamExp()
            x.resolvable = False
        else:
            x = walk_stream(flat, b, e)
            inside = [c for c in mine if c < e]
            chain = set(x.units) | {g.off for g in x.live}
            cset = set(inside)
            own = tuple(x.sync[k] for k in ("group0_bps", "group1_bps", "group0_rate", "group1_rate", "assignment"))
            false = [c for c in inside if c not in chain]
            starts = np.asarray([g.off for g in x.live], np.int64)
            per_seg = np.zeros(len(x.live), np.int64)
            for c in false:
                if _own_walk_lands(flat, c, e, cset):
                    x.resolvable = False
                if sync_params(flat, c) == own:
                    per_seg[np.searchsorted(starts, c, "right") - 1] += 1
            if per_seg.max(initial=0) > MAX_DROP:
                x.resolvable = False
            # `segments` as the library reports it today: the stream's run in the candidate list -- its own range's
            # candidates, retired ones included, and those in nobody's bytes behind it (they are looked up to it)
            x.segments = len(mine)
            for g in x.live:
                ix.seg[index_of[g.off]] = g
        ix.streams.append(x)
    return ix


def compare(ix, infos, segment_info=None, sample=None):
    """Asserts what the library reported (infos: dvda_mlp_stream_info per stream after an index without a decode;
    segment_info: a function of the segment index) against the model.  sample: the segment indices to read (None:
    all of them)."""
    for s, (x, inf) in enumerate(zip(ix.streams, infos)):
        st = int(inf.status)
        if x.capacity:
            assert st & CAPACITY, "stream %d: behind the cut without DVDA_ST_CAPACITY (%#x)" % (s, st)
            continue
        assert not st & CAPACITY, "stream %d: in front of the cut, yet DVDA_ST_CAPACITY (%#x)" % (s, st)
        if not x.resolvable:
            assert st & IRREGULAR, "stream %d: not resolvable, yet no DVDA_ST_IRREGULAR (%#x)" % (s, st)
            continue
        got = (int(inf.mlp_frames), int(inf.bytes_consumed), int(inf.segments), st)
        want = (x.mlp_frames, x.bytes_consumed, x.segments, x.status)
        assert got == want, "stream %d: (frames, consumed, segments, status) %r, model %r" % (s, got, want)
        if x.sync:
            assert {k: int(getattr(inf, k)) for k in x.sync} == x.sync, "stream %d: sync fields" % s
    if segment_info is None:
        return
    owner = np.searchsorted(np.asarray(ix.soff, np.int64), ix.cands, "right") - 1
    for i in (range(len(ix.cands)) if sample is None else sample):
        s = int(owner[i])
        if s >= 0 and (ix.streams[s].capacity or not ix.streams[s].resolvable):
            continue
        r = segment_info(i)
        assert int(r.offset) == int(ix.cands[i]), "segment %d at %d, model %d" % (i, r.offset, ix.cands[i])
        g = ix.seg[i]
        if g is None:
            assert int(r.status) & FALSE_SYNC and int(r.mlp_frames) == 0, \
                "segment %d (offset %d) is not retired: %#x, %d frames" % (i, r.offset, r.status, r.mlp_frames)
        else:
            got = (int(r.offset), int(r.end), int(r.mlp_frames), int(r.status) & INDEX_BITS)
            assert got == g.record() and int(r.stream) == s, "segment %d: %r, model %r" % (i, got, g.record())


# ------------------------------------------------------------------------------------------------ case builders

def unit_offsets(stream):
    return stream_tools.frame_offsets(stream)


def fake_sync(params, substreams, size_words):
    """the 32 bytes of a major-sync access unit header with the five parameters `params`"""
    f = np.zeros(32, np.uint8)
    f[0], f[1] = (size_words >> 8) & 0x0F, size_words & 0xFF
    f[4:8] = [0xF8, 0x72, 0x6F, 0xBB]
    f[8] = (params[0] << 4) | params[1]
    f[9] = (params[2] << 4) | params[3]
    f[11] = params[4]
    f[20] = substreams << 4
    return f


def with_false_syncs(stream, unit, n, params=None, size_words=0x40, stride=64, substreams=None):
    """`stream` with access unit `unit` grown by n * stride ignored tail bytes (the reference ignores what follows a
    unit's last substream, src/mlp.c:463-610), every `stride` of them beginning with the header of a major-sync
    access unit.  params: its five stream parameters (None: the stream's own); size_words: its size field."""
    b = np.asarray(stream, np.uint8)
    offs = unit_offsets(b)
    pos = offs[unit]
    size = unit_size(b, pos)
    assert stride >= 32 and stride % 2 == 0
    tail = np.zeros(n * stride, np.uint8)
    f = fake_sync(sync_params(b, 0) if params is None else params,
                  int(b[20]) >> 4 if substreams is None else substreams, size_words)
    for k in range(n):
        tail[k * stride:k * stride + 32] = f
    new_size = size + len(tail)
    assert new_size <= 8190, "an access unit holds 4095 words"
    out = np.concatenate([b[:pos + size], tail, b[pos + size:]])
    out[pos] = (int(b[pos]) & 0xF0) | ((new_size // 2) >> 8)
    out[pos + 1] = (new_size // 2) & 0xFF
    return out


def inject_false_sync(stream, frame_index):
    """one access unit grown by 64 ignored tail bytes that look exactly like the header of a major-sync access unit
    of a 6-channel 96 kHz stream with a size field of 128 bytes (tests/test_gpu_parity.py's case since round 1)"""
    return with_false_syncs(stream, frame_index, 1, params=(2, 2, 1, 1, 12), size_words=0x40, stride=64, substreams=1)


def place_sync(stream, base, which, target):
    """`stream`, which starts at absolute offset `base`, with the access unit in front of its `which`-th major sync
    padded so that this major sync starts at absolute offset `target`"""
    syncs = stream_tools.major_syncs(stream)
    units = unit_offsets(stream)
    p = syncs[which]
    u = units.index(p) - 1
    assert u >= 0
    grow = target - (base + p)
    assert grow >= 0 and grow % 2 == 0
    if grow == 0:
        return stream
    out = stream_tools.padded_unit(stream, u, unit_size(stream, units[u]) + grow)
    assert stream_tools.major_syncs(out)[which] == target - base
    return out


def start_for(target, first_unit):
    """the 16-byte aligned start of a stream whose first unit (first_unit bytes, to be padded by 2 .. 17) is to end
    at `target`"""
    return (target - first_unit - 2) & ~15


def phases_stream(stream):
    """`stream` (a major sync in every unit, nine or more of them) padded so that its first nine major syncs start at
    phases 0, 2, .., 14, 0 of a 16-byte chunk"""
    out = stream
    for k in range(1, 9):
        at = stream_tools.major_syncs(out)[k]
        out = place_sync(out, 0, k, at + ((2 * k - at) % 16 or 16))
    return out


def cut_tail(stream, short):
    return np.ascontiguousarray(stream[:len(stream) - short])


def cut_in_last_sync(stream, keep=20):
    """the stream cut `keep` bytes into its last major-sync access unit (32 or more: the major sync stands whole)"""
    return np.ascontiguousarray(stream[:stream_tools.major_syncs(stream)[-1] + keep])


def lay_out(streams, starts=None, total=None, spare=64):
    """-> (flat with `spare` readable bytes behind total, offs, lens, total): streams at the given absolute starts
    (None: packed end to end, 16-byte aligned)"""
    if starts is None:
        starts, pos = [], 0
        for s in streams:
            starts.append(pos)
            pos += (len(s) + 15) & ~15
    end = max([o + len(s) for o, s in zip(starts, streams)] + [0])
    total = end if total is None else total
    assert total >= end and all(o % 16 == 0 for o in starts)
    flat = np.zeros(total + spare, np.uint8)
    for o, s in zip(starts, streams):
        assert not flat[o:o + len(s)].any(), "streams overlap"
        flat[o:o + len(s)] = s
    return flat, np.asarray(starts, np.uint64), np.asarray([len(s) for s in streams], np.uint64), total


def single(stream):
    """the model's records for one stream alone in its buffer"""
    flat, offs, lens, total = lay_out([stream])
    return expect(flat, total, offs, lens).streams[0]


def benign_cases(syn):
    """[(name, stream bytes, channels, rate code, resolvable)]: streams the reference decodes (to the end, or to the
    cut); all but the last two are in the resolvable class by construction"""
    cfg = syn.make_cfg(assignment=1, rate_code=0, n_aus=24, restart_interval=4)
    clean, _ = syn.stream(cfg, 4101)
    cfg1 = syn.make_cfg(assignment=1, rate_code=0, n_aus=80, restart_interval=1)
    every, _ = syn.stream(cfg1, 4102)
    cfg6 = syn.make_cfg(assignment=12, rate_code=1, n_aus=12, restart_interval=3)
    six, _ = syn.stream(cfg6, 4103)
    foreign = (2, 2, 1, 1, 12)
    cases = [("clean", clean, 2, 0), ("clean-6ch", six, 6, 1), ("every-unit-a-sync", every, 2, 0),
             ("phases", phases_stream(every), 2, 0),
             ("padded-3", stream_tools.padded_unit(clean, 3, unit_size(clean, unit_offsets(clean)[3]) + 700), 2, 0)]
    for short in (1, 3, 4, 31, 33, 123):
        cases.append(("cut-%d" % short, cut_tail(clean, short), 2, 0))
    cases.append(("cut-in-last-sync", cut_in_last_sync(clean), 2, 0))
    for keep in (30, 32, 34):
        cases.append(("cut-%d-into-last-sync" % keep, cut_in_last_sync(clean, keep), 2, 0))
    cases.append(("cut-34-into-changed-sync",
                  cut_in_last_sync(stream_tools.change_sync_params(clean, (5,), g1_bps=0)[0], 34), 2, 0))
    cases.append(("changed-1",stream_tools.change_sync_params(clean, (2,), g1_bps=0)[0], 2, 0))
    cases.append(("changed-5-in-a-row", stream_tools.change_sync_params(every, tuple(range(3, 8)), assignment=3)[0], 2, 0))
    cases.append(("changed-70-in-a-row", stream_tools.change_sync_params(every, tuple(range(2, 72)), g1_bps=0)[0], 2, 0))
    for n in (1, 8, 64):
        for unit in (0, 9, 23):
            cases.append(("own-false-%d-unit-%d" % (n, unit), with_false_syncs(clean, unit, n, None, 0x11, 40), 2, 0))
    cases.append(("foreign-false-200", with_false_syncs(clean, 5, 200, foreign, 0x11, 36), 2, 0))
    cases.append(("false-past-the-end", with_false_syncs(clean, 20, 3, None, 0xFFF, 40), 2, 0))
    cases.append(("parity-case-false-sync", inject_false_sync(six, 3), 6, 1))
    out = [(name, b, nch, rate, True) for name, b, nch, rate in cases]
    # benign for the reference, not resolvable for the index: 200 own-parameter false syncs in one segment; false
    # syncs 32 bytes apart whose size field (128 bytes) lands each on the fourth behind it
    out.append(("own-false-200", with_false_syncs(clean, 5, 200, None, 0x11, 36), 2, 0, False))
    out.append(("chained-false-8", with_false_syncs(clean, 5, 8, None, 0x40, 32), 2, 0, False))
    for name, b, nch, rate, resolvable in out:
        assert single(b).resolvable == resolvable, "%s is built for the other class" % name
    return out
