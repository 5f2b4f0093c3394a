"""The presentation strip on the GPU (csrc/mlp_present.h, csrc/mlp_present_run.h) at its edges: every case of
tests/presentation_cases.py is indexed under DVDA_PRESENT_SUBSTREAM0 and the presentation buffer, read back with
dvda_mlp_hip_present_read, is held to the model's byte for byte -- the streams' lengths and offsets, the zero padding
behind each stream and the zeros behind the last one up to what the second index may read included.  The decodable
cases are decoded too: PCM and every stream_info field against tests/presentation_model.py and tests/index_model.py.
Everything is exact.  (The premises of the cases -- which pairs, classes and clamps they reach -- are asserted on the CPU,
tests/test_presentation_cases_model.py.)"""
import numpy as np
import pytest

from tests import index_model as im
from tests import presentation_cases as pc
from tests import presentation_model as pm

pytestmark = pytest.mark.gpu

EINVAL = -3
INFO_FIELDS = ("mlp_frames", "pcm_frames", "bytes_consumed", "channels", "substreams", "assignment", "group0_bps",
               "group1_bps", "group0_rate", "group1_rate", "segments")


def _segments_for(flat, total):
    return max(64, len(im.candidates(flat, total)) + 7)


def _describe(b, at):
    """where byte `at` of the presentation buffer belongs: the stream, and for a two-substream stream the unit, its body's
    (dst phase, src - dst phase) pair and class"""
    _, poffs, plens, _ = pc.present_buffer(b)
    i = int(np.searchsorted(np.asarray(poffs), at, "right")) - 1
    text = "byte %d: stream %d (at %d, %d bytes)" % (at, i, poffs[i], plens[i])
    if len(b.streams) > 64:
        return text
    for r in pc.walk(b):
        if r.stream == i and r.dst - 4 - r.sync - r.dir0 <= at < r.dst + r.n:
            return text + ", unit %d (sync %d, directory %d + %d): %s of a body of %d bytes, pair %r, class %s" % (
                r.unit, r.sync, r.dir0, r.dir1, "byte %d" % (at - r.dst) if at >= r.dst else "header", r.n, pc.pair(r),
                pc.body_class(r.n, r.dst))
    return text


def check_bytes(ctx, b, st=0):
    """the presentation buffer of the context's last index against the model's"""
    buf, poffs, plens, bound = pc.present_buffer(b)
    offs, lens, readable, data = ctx.present_read(stream=st)
    assert readable == bound + 64 and len(data) == readable
    assert lens.tolist() == plens, "stream lengths: first difference at stream %d" % int(np.flatnonzero(lens != np.asarray(plens, np.uint64))[0])
    starts = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 15) & ~15)])
    assert offs.tolist() == starts[:-1].tolist(), "every stream starts at the running sum of the lengths rounded up to 16"
    ends = offs.astype(np.int64) + lens.astype(np.int64)
    pad = np.zeros(len(data), bool)
    for e, nxt in zip(ends.tolist(), starts[1:].tolist()):
        if nxt > e:
            pad[e:nxt] = True
    assert not data[pad].any(), "padding behind a stream: " + _describe(b, int(np.flatnonzero(pad & (data != 0))[0]))
    used = int(starts[-1])
    assert not data[used:].any(), "byte %d behind the last stream (which ends at %d; readable %d) is not zero" % (
        used + int(np.flatnonzero(data[used:])[0]), used, readable)
    wrong = np.flatnonzero(data != buf)
    assert not len(wrong), "%d bytes differ from the model; the first: %s" % (len(wrong), _describe(b, int(wrong[0])))
    return data


def check_inner_index(ctx, b, st=0, segments=False):
    """the second index's records against index_model.expect over the model's presentation buffer: mlp_frames and
    segments per stream that has a presentation; segments=True: every segment's frames, retired or live"""
    ix = pc.inner_index(b)
    _, _, plens, _ = pc.present_buffer(b)
    infos = ctx.stream_info(stream=st)
    assert ctx.segment_count(st) == ix.n_found
    got = [(int(inf.mlp_frames), int(inf.segments)) for inf, n in zip(infos, plens) if n]
    want = [(x.mlp_frames, x.segments) for x, n in zip(ix.streams, plens) if n]
    assert all(x.resolvable for x, n in zip(ix.streams, plens) if n)
    assert got == want, "(mlp_frames, segments): first difference at presentation stream %d" % next(
        i for i, (g, w) in enumerate(zip(got, want)) if g != w)
    if segments:
        for j in range(ix.n_found):
            r = ctx.segment_info(j, st)
            g = ix.seg[j]
            if g is None:
                assert r.status & im.FALSE_SYNC and int(r.mlp_frames) == 0, "segment %d is not retired" % j
            else:
                assert int(r.mlp_frames) == g.nframes and not r.status & im.FALSE_SYNC, "segment %d" % j
    return infos


def index_only(pkg, b):
    hd = pkg.hipdec
    flat, offs, lens, total = pc.source(b)
    batch = hd.Batch(packed=(flat, offs, lens))
    ctx = hd.Context(0, len(offs), _segments_for(flat, total))
    try:
        ctx.set_presentation(hd.PRESENT_SUBSTREAM0)
        ctx.index_batch(batch)
        check_bytes(ctx, b)
        check_inner_index(ctx, b)
    finally:
        ctx.close()


def check_decoded(hd, oracle, b, pcm, infos, full=None):
    """every stream of a decodable batch against the model, by its kind; full: the stream_info of the same batch indexed
    under DVDA_PRESENT_FULL (what a stream without a presentation keeps)"""
    for i, (kind, inf, got) in enumerate(zip(b.decode["kinds"], infos, pcm)):
        st = int(inf.status)
        if kind in ("good", "cut"):
            want, wpcm = pc.expected_info(b, i, oracle)
            have = {f: int(getattr(inf, f)) for f in INFO_FIELDS}
            have["status"] = st & (im.TRUNCATED | im.SYNC_CHANGE)
            assert have == want, "stream %d (%s)" % (i, kind)
            assert st & ~hd.ST_BENIGN == 0, "stream %d (%s): status %#x" % (i, kind, st)
            assert got.shape == wpcm.shape and np.array_equal(got, wpcm), "stream %d (%s): PCM differs from the model" % (i, kind)
            continue
        s = b.streams[i]
        assert (int(inf.mlp_frames), int(inf.pcm_frames), int(inf.segments)) == (0, 0, 0) and got.size == 0, i
        f = full[i]
        for name in ("substreams", "assignment", "group0_bps", "group1_bps", "group0_rate", "group1_rate", "bytes_consumed"):
            assert int(getattr(inf, name)) == int(getattr(f, name)), "stream %d (%s): %s" % (i, kind, name)
        if kind == "envelope":
            assert st == int(f.status) | pm.ST_ENVELOPE and int(f.status) & ~hd.ST_BENIGN == 0, "stream %d: %#x" % (i, st)
            assert int(inf.channels) == 0 and int(inf.bytes_consumed) == pm.consumed(s) and int(inf.substreams) == 2
        else:
            assert st & ~im.NO_SYNC == int(f.status) & ~im.NO_SYNC, "stream %d: %#x, full %#x" % (i, st, int(f.status))
            assert st & (im.NO_SYNC | im.IRREGULAR | im.CAPACITY), "stream %d: %#x" % (i, st)
            assert int(inf.channels) == int(f.channels) and int(inf.bytes_consumed) == 0


def decode_case(pkg, oracle, b, layout, lanes, segments=False, full=False):
    hd = pkg.hipdec
    flat, offs, lens, total = pc.source(b)
    batch = hd.Batch(packed=(flat, offs, lens))
    ms = _segments_for(flat, total)
    finfos = None
    if full:
        ctx = hd.Context(0, len(offs), ms)
        try:
            ctx.index_batch(batch)
            finfos = list(ctx.stream_info())
        finally:
            ctx.close()
    ctx = hd.Context(0, len(offs), ms, lanes, layout)
    try:
        ctx.set_presentation(hd.PRESENT_SUBSTREAM0)
        pcm, infos, _ = hd.decode_batch(ctx, batch, layout)
        check_bytes(ctx, b, batch.current_stream)
        check_inner_index(ctx, b, batch.current_stream, segments)
        check_decoded(hd, oracle, b, pcm, infos, finfos)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ bytes and index only

def test_copy_sweep(pkg):
    """(a) every (dst phase, src - dst phase) pair and every body class of pp_copy, both directory sizes of both
    substreams on sync and plain units; a wrong byte is named by pair and class"""
    index_only(pkg, pc.batch(pkg.synth, "sweep"))


def test_clamps(pkg):
    """(b) units that end before or inside their directory, substream ends beyond the unit, an extra-word flag on the
    unit's last two bytes"""
    index_only(pkg, pc.batch(pkg.synth, "clamps"))


@pytest.mark.parametrize("n", [255, 256, 257, 1025, 16385])
def test_launch_geometry(pkg, n):
    """(g) the second block of k_pp_streams / k_pp_len, both forms of the two scans, and with 16 385 single-unit streams
    the stride loop of k_pp_copy beyond its 16 384 waves"""
    index_only(pkg, pc.batch(pkg.synth, "geometry%d" % n))


# ------------------------------------------------------------------------------------------------ decoded

@pytest.mark.parametrize("lanes", [0, 3])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_large_bodies(pkg, oracle, layout, lanes):
    """(c) bodies of more than 64 and more than 128 whole chunks on streams that decode"""
    hd = pkg.hipdec
    decode_case(pkg, oracle, pc.batch(pkg.synth, "large"), hd.PCM_PLANAR if layout == "planar" else hd.PCM_INTERLEAVED, lanes)


def test_one_substream_streams(pkg, oracle):
    """(d) the k == 0 path: segments over 1 KB at all eight phases; the presentation is the source's complete units"""
    decode_case(pkg, oracle, pc.batch(pkg.synth, "one_substream"), pkg.hipdec.PCM_PLANAR, 0)


def test_mixed_findings_in_one_batch(pkg, oracle):
    """(e) PP_NONE, a stream of no bytes, PP_ENVELOPE twice and four cuts inside the last unit, good streams around each"""
    decode_case(pkg, oracle, pc.batch(pkg.synth, "mixed"), pkg.hipdec.PCM_PLANAR, 0, full=True)


@pytest.mark.parametrize("lanes", [0, 3])
def test_sync_edges(pkg, oracle, lanes):
    """(f) false syncs behind and inside substream 0, a major sync that differs in the assignment alone (decoded here,
    dropped by the full decode) and in a group code (dropped in both), a SYNCONLY stream"""
    hd = pkg.hipdec
    b = pc.batch(pkg.synth, "sync")
    decode_case(pkg, oracle, b, hd.PCM_PLANAR, lanes, segments=True)
    if lanes == 0:
        _, infos = hd.decode_streams([b.streams[2]])
        assert int(infos[0].pcm_frames) == 1840 and infos[0].status & im.SYNC_CHANGE       # the full decode drops the unit


# ------------------------------------------------------------------------------------------------ one context, batches

def _run_step(hd, ctx, b, mode):
    flat, offs, lens, total = pc.source(b)
    batch = hd.Batch(packed=(flat, offs, lens))
    ctx.set_presentation(mode)
    pcm, infos, _ = hd.decode_batch(ctx, batch, hd.PCM_PLANAR)
    st = batch.current_stream
    segs = [ctx.segment_info(j, st) for j in range(ctx.segment_count(st))]
    return batch, pcm, infos, segs


@pytest.mark.parametrize("seq", list(pc.REUSE_SEQUENCES))
def test_one_context_several_batches(pkg, oracle, seq):
    """(h) the presentation buffer reused: after a small batch behind a big one every byte behind its last stream is zero
    (the big batch left major syncs there), the buffer grows behind a small one, and the mode switched off and on again
    between two batches; the last batch comes out as on a fresh context"""
    hd, syn = pkg.hipdec, pkg.synth
    steps = pc.REUSE_SEQUENCES[seq]
    ctx = hd.Context(0, 8, 4096)
    try:
        for name, mode in steps:
            b = pc.batch(syn, name)
            batch, pcm, infos, segs = _run_step(hd, ctx, b, mode)
            if mode:
                check_bytes(ctx, b, batch.current_stream)
                check_inner_index(ctx, b, batch.current_stream)
                check_decoded(hd, oracle, b, pcm, infos)
            else:
                assert all(inf.status & ~hd.ST_BENIGN == 0 and int(inf.channels) == 6 for inf in infos)
                with pytest.raises(hd.HipError, match="ESTATE"):
                    ctx.present_read()
    finally:
        ctx.close()
    fresh = hd.Context(0, 8, 4096)
    try:
        _, fpcm, finfos, fsegs = _run_step(hd, fresh, b, 1)
    finally:
        fresh.close()
    fields = [f for f, _ in hd.StreamInfo._fields_]
    assert len(pcm) == len(fpcm) and all(np.array_equal(x, y) for x, y in zip(pcm, fpcm))
    assert [[int(getattr(x, f)) for f in fields] for x in infos] == [[int(getattr(x, f)) for f in fields] for x in finfos]
    sfields = [f for f, _ in hd.SegmentInfo._fields_]
    assert [[int(getattr(x, f)) for f in sfields] for x in segs] == [[int(getattr(x, f)) for f in sfields] for x in fsegs]


# ------------------------------------------------------------------------------------------------ the getter

def test_present_read_states_ranges_and_leaves_the_context_alone(pkg, oracle):
    hd = pkg.hipdec
    b = pc.batch(pkg.synth, "reuse_small")
    flat, offs, lens, total = pc.source(b)
    batch = hd.Batch(packed=(flat, offs, lens))
    ctx = hd.Context(0, 1, 64)
    try:
        for prepare in (lambda: None, lambda: ctx.set_presentation(hd.PRESENT_SUBSTREAM0), lambda: (
                ctx.set_presentation(hd.PRESENT_FULL), ctx.index_batch(batch))):
            prepare()
            with pytest.raises(hd.HipError, match="ESTATE"):
                ctx.present_read()
        ctx.set_presentation(hd.PRESENT_SUBSTREAM0)
        with pytest.raises(hd.HipError, match="ESTATE"):                     # the change of the setting asks for a new index
            ctx.present_read()
        ctx.index_batch(batch)
        fields = [f for f, _ in hd.StreamInfo._fields_]
        before = [int(getattr(ctx.stream_info()[0], f)) for f in fields]
        data = check_bytes(ctx, b)
        readable = len(data)
        for first, count in ((0, 0), (readable, 0), (0, 1), (readable - 1, 1), (30, 4000), (3391, 77)):
            _, _, r, part = ctx.present_read(first, count)
            assert r == readable and np.array_equal(part, data[first:first + count]), (first, count)
        L = hd.lib()
        one = np.zeros(8, np.uint8)
        assert L.dvda_mlp_hip_present_read(ctx._h, None, None, 0, None, one.ctypes.data, readable, 1, 0) == EINVAL
        assert L.dvda_mlp_hip_present_read(ctx._h, None, None, 0, None, one.ctypes.data, readable + 1, 0, 0) == EINVAL
        assert L.dvda_mlp_hip_present_read(ctx._h, None, None, 0, None, one.ctypes.data, 1, 2 ** 64 - 1, 0) == EINVAL
        assert L.dvda_mlp_hip_present_read(ctx._h, None, None, 0, None, None, 0, 1, 0) == EINVAL
        assert L.dvda_mlp_hip_present_read(None, None, None, 0, None, None, 0, 0, 0) == EINVAL
        assert not one.any()
        assert [int(getattr(ctx.stream_info()[0], f)) for f in fields] == before
        # the decode behind the reads is the decode without them
        regions = hd.PcmRegions.for_infos(ctx.stream_info())
        ctx.decode(*regions.ptrs, 0)
        infos = ctx.stream_info()
        check_decoded(hd, oracle, b, regions.to_host(infos), infos)
        check_bytes(ctx, b)
    finally:
        ctx.close()
