"""The GPU frame index (csrc/mlp_index.h, k_check_ranges, k_au_check) against the serial model of tests/index_model.py,
at the positions where its kernels change path: the phases of a 16-byte chunk, a scatter thread's 256 bytes, a wave's
16 KiB, the 64 KiB tile, the ragged last chunk, both forms of every scan, the capacity cut, more than 1024 streams,
the lane packing as a permutation, the index replayed as a hipGraph, and the substream checks by position.
Resolvable streams are asserted exactly, the others "flagged" (index_model's two classes).  Index-only unless a decode
is named."""
import numpy as np
import pytest

from tests import index_model as im
from tests import stream_tools

pytestmark = pytest.mark.gpu

FOREIGN = (2, 2, 1, 1, 12)          # parameters no 2-channel 48 kHz stream announces


@pytest.fixture(scope="module")
def every(pkg):
    """2-channel 48 kHz, twelve units of 302 bytes, a major sync in each"""
    return pkg.synth.stream(pkg.synth.make_cfg(assignment=1, rate_code=0, n_aus=12, restart_interval=1), 5101)[0]


@pytest.fixture(scope="module")
def clean(pkg):
    """2-channel 48 kHz, 24 units in six segments"""
    return pkg.synth.stream(pkg.synth.make_cfg(assignment=1, rate_code=0, n_aus=24, restart_interval=4), 4101)[0]


def _index_exact(hip, flat, offs, lens, max_segments=None, sample=None, ix=None):
    """index (no decode) on a fresh context and hold every record to the model"""
    total = len(flat) - 64
    ix = im.expect(flat, total, offs, lens, max_segments) if ix is None else ix
    batch = hip.Batch(packed=(flat, offs, lens))
    ctx = hip.Context(0, len(offs), max_segments or max(64, ix.n_found + 7))
    try:
        ctx.index_batch(batch)
        if ix.overflow:
            with pytest.raises(hip.HipError):
                ctx.segment_count()
        else:
            assert ctx.segment_count() == ix.n_found
        im.compare(ix, ctx.stream_info(), ctx.segment_info, sample)
    finally:
        ctx.close()
    return ix


def _decode_against_oracle(hip, oracle, flat, offs, lens, nch, rates, ix, layout=None, ctx=None, stream=None,
                           cache=None):
    """decode the batch and hold every resolvable stream's PCM to the oracle's; the others must be flagged"""
    layout = hip.PCM_PLANAR if layout is None else layout
    batch = flat if isinstance(flat, hip.Batch) else hip.Batch(packed=(flat, offs, lens))
    own = ctx is None
    ctx = hip.Context(0, len(offs), max(64, ix.n_found + 7), 0, layout) if own else ctx
    try:
        pcm, infos, _ = hip.decode_batch(ctx, batch, layout, stream=stream)
    finally:
        if own:
            ctx.close()
    host = flat if not isinstance(flat, hip.Batch) else None
    for s, (x, inf, got) in enumerate(zip(ix.streams, infos, pcm)):
        if not x.resolvable or x.refused:
            assert inf.status & im.IRREGULAR and (inf.status & ~hip.ST_BENIGN), "stream %d: %#x" % (s, inf.status)
            continue
        key = None
        if cache is not None:
            key = cache["key"][s]
        if key is None or key not in cache:
            b = host[int(offs[s]):int(offs[s]) + int(lens[s])]
            want = oracle.decode(b, nch[s], (x.mlp_frames + 2) * im.ROWS_PER_AU[rates[s]])
            if key is not None:
                cache[key] = want
        else:
            want = cache[key]
        w, r, st = want
        assert r == x.mlp_frames * im.ROWS_PER_AU[rates[s]] and not st & ~2
        assert inf.status & ~hip.ST_BENIGN == 0, "stream %d: status %#x" % (s, inf.status)
        assert int(inf.pcm_frames) == r and int(inf.mlp_frames) == x.mlp_frames, "stream %d" % s
        assert got.shape == w.shape and np.array_equal(got, w), "stream %d: PCM differs" % s
    return infos


# ------------------------------------------------------------------------------------------------ sync positions

def _steered(every):
    """28 streams: one with its major syncs at all eight phases of a chunk; for B = a scatter thread's 256-byte run,
    a wave's 16 KiB and the 64 KiB tile, nine streams whose second major sync starts at B - 16, B - 14, .., B (the
    pattern bytes p + 4 .. p + 7 lie across B for B - 6, wholly behind it from B - 4 on)"""
    first = im.unit_size(every, 0)
    streams, starts, aimed = [], [], []
    region = 0
    for G in (256, 16384, 65536):
        for k in range(9):
            B = region + (G if G != 256 else 256 * ((first + 18 + 255) // 256))
            t = B - 16 + 2 * k
            base = im.start_for(t, first)
            assert base >= region
            streams.append(im.place_sync(every, base, 1, t))
            starts.append(base)
            aimed.append(t)
            region += 131072
    streams.append(im.phases_stream(every))
    starts.append(region)
    return streams, starts, aimed


@pytest.mark.parametrize("ragged", [0, 10])
def test_major_syncs_at_every_phase_and_across_every_boundary(pkg, oracle, every, ragged):
    hip = pkg.hipdec
    streams, starts, aimed = _steered(every)
    end = starts[-1] + len(streams[-1])
    flat, offs, lens, total = im.lay_out(streams, starts, total=((end + 15) & ~15) + ragged)
    assert total % 16 == ragged
    ix = im.expect(flat, total, offs, lens)
    for s, t in enumerate(aimed):
        assert ix.streams[s].resolvable and ix.streams[s].live[1].off == t and ix.streams[s].mlp_frames == 12
    assert [g.off % 16 for g in ix.streams[-1].live[:9]] == [0, 2, 4, 6, 8, 10, 12, 14, 0]
    _index_exact(hip, flat, offs, lens, ix=ix)
    _decode_against_oracle(hip, oracle, flat, offs, lens, [2] * len(streams), [0] * len(streams), ix)


def test_sync_pattern_in_front_of_the_first_stream_is_nobodys(pkg, oracle, every):
    """bytes in front of the first stream's range belong to no stream: a sync pattern there is retired and the
    first stream comes out exact (the stream look-up gives such an offset to stream 0)"""
    hip = pkg.hipdec
    flat, offs, lens, total = im.lay_out([every, every], [4096, 8192])
    flat[64:96] = im.fake_sync(im.sync_params(every, 0), 1, 0x11)
    flat[1026:1058] = im.fake_sync(FOREIGN, 1, 0x40)
    ix = im.expect(flat, total, offs, lens)
    assert ix.n_found == 26 and ix.seg[0] is None and ix.seg[1] is None and ix.streams[0].segments == 12
    _index_exact(hip, flat, offs, lens, ix=ix)
    _decode_against_oracle(hip, oracle, flat, offs, lens, [2, 2], [0, 0], ix)


@pytest.mark.parametrize("d", [30, 32, 34])
def test_ragged_total_and_a_major_sync_at_the_end_of_the_buffer(pkg, oracle, every, clean, d):
    """total_bytes no multiple of 16 and the last stream's last major sync d bytes in front of it: with 30 the
    pattern is no candidate (the sync test needs 32 bytes), from 32 on it opens a segment of no units; the same cut
    by a stream's range in the middle of the buffer, behind an own and behind a changed major sync"""
    hip = pkg.hipdec
    changed = stream_tools.change_sync_params(clean, (5,), g1_bps=0)[0]
    last = stream_tools.major_syncs(clean)[-1]
    streams = [clean, clean, changed, every, clean]
    flat, offs, lens, _ = im.lay_out(streams)
    lens = lens.copy()
    lens[1] = last + 34             # the range ends inside the unit; its bytes go on behind the range (nobody's)
    lens[2] = last + 34
    lens[4] = last + d
    total = int(offs[4]) + last + d
    flat = np.concatenate([flat[:total], np.zeros(64, np.uint8)])       # 64 readable spare bytes, nothing in them
    assert total % 16 != 0
    ix = im.expect(flat, total, offs, lens)
    want_last = (im.TRUNCATED, 20, 5 if d == 30 else 6)
    assert (ix.streams[4].status, ix.streams[4].mlp_frames, ix.streams[4].segments) == want_last
    assert ix.streams[1].live[-1].record() == (int(offs[1]) + last, int(offs[1]) + last, 0, im.TRUNCATED)
    assert ix.streams[2].status == im.TRUNCATED and ix.streams[2].mlp_frames == 20      # the cut unit is not dropped: not read
    assert ix.streams[0].status == 0 and ix.streams[3].status == 0
    _index_exact(hip, flat, offs, lens, ix=ix)
    _decode_against_oracle(hip, oracle, flat, offs, lens, [2] * 5, [0] * 5, ix)


# ------------------------------------------------------------------------------------------------ dense candidates

def test_dense_false_candidates_in_many_lanes_and_across_a_tile(pkg, oracle, clean):
    hip = pkg.hipdec
    own64 = im.with_false_syncs(clean, 9, 64, None, 0x11, 40)
    foreign200 = im.with_false_syncs(clean, 5, 200, FOREIGN, 0x11, 36)
    own200 = im.with_false_syncs(clean, 5, 200, None, 0x11, 36)
    chained = im.with_false_syncs(clean, 5, 8, None, 0x40, 32)
    u = im.unit_offsets(clean)
    # own64's false syncs (2560 bytes behind unit 9) across a wave's 16 KiB boundary, foreign200's (7200 bytes behind
    # unit 5) across the tile boundary at 64 KiB
    streams = [clean, own200, own64, chained, foreign200, clean]
    starts = [0, 8192, (32768 - 1280 - u[10]) & ~15, 40960, (65536 - 3600 - u[6]) & ~15, 81920]
    flat, offs, lens, total = im.lay_out(streams, starts)
    ix = im.expect(flat, total, offs, lens)
    assert [x.resolvable for x in ix.streams] == [True, False, True, False, True, True]
    false64 = [c for i, c in enumerate(ix.cands.tolist()) if ix.seg[i] is None and starts[2] <= c < starts[3]]
    false200 = [c for i, c in enumerate(ix.cands.tolist()) if ix.seg[i] is None and starts[4] <= c < starts[5]]
    assert len(false64) == 64 and false64[0] < 32768 < false64[-1]
    assert len(false200) == 200 and false200[0] < 65536 < false200[-1]
    assert ix.streams[2].segments == 70 and ix.streams[4].segments == 206 and ix.streams[2].status == 0
    _index_exact(hip, flat, offs, lens, ix=ix)
    _decode_against_oracle(hip, oracle, flat, offs, lens, [2] * 6, [0] * 6, ix)


# ------------------------------------------------------------------------------------------------ the scans

@pytest.fixture(scope="module")
def batch_1024x4(pkg):
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=1, rate_code=0, n_aus=8, restart_interval=2)
    buf, off, siz, _ = syn.batch(cfg, 7000, 1024)
    return buf, off.astype(np.int64), siz.astype(np.int64)


@pytest.mark.parametrize("n_cand", [1, 1023, 1024, 1025, 2049, 4096])
def test_both_forms_of_the_segment_scan(pkg, batch_1024x4, n_cand):
    """prefixes of 1024 streams x 4 segments with n_cand candidates, each through contexts whose max_segments puts
    the scan of the segments' frame counts on either side of its switch at 4096 (and the multi-block form at five and
    nine blocks)"""
    hip = pkg.hipdec
    buf, off, siz = batch_1024x4
    q, r = divmod(n_cand, 4)
    n = q + (1 if r else 0)
    offs, lens = off[:n].copy(), siz[:n].copy()
    if r:
        s = buf[off[q]:off[q] + siz[q]]
        lens[q] = stream_tools.major_syncs(s)[r]            # the range ends in front of the stream's (r + 1)-th sync
    total = int(offs[-1] + lens[-1])
    flat = np.concatenate([buf[:total], np.zeros(64, np.uint8)])
    ix = im.expect(flat, total, offs, lens)
    assert ix.n_found == n_cand and all(x.resolvable for x in ix.streams)
    assert all(x.mlp_frames == 8 and x.segments == 4 for x in ix.streams[:q])
    sample = sorted({i for i in (0, 1023, 1024, 1025, n_cand - 1) if i < n_cand})
    for ms in (4096, 4097, 8193):
        _index_exact(hip, flat, offs, lens, max_segments=ms, sample=sample, ix=ix)


def test_tile_count_scan_above_4096_tiles(pkg, every):
    """4097 tiles and a ragged chunk of zeros: short streams at the start, across the tile boundary 4095 | 4096 and
    at the very end, one sync pattern in nobody's bytes.  (The only case above a few MiB.)"""
    hip = pkg.hipdec
    total = 4097 * 65536 + 40
    n = len(every)
    starts = [0, (4096 * 65536 - n // 2) & ~15, (total - n) & ~15]
    streams = [every, every, every[:total - starts[2]]]
    flat, offs, lens, total = im.lay_out(streams, starts, total=total)
    lone = 2000 * 65536 + 0x1234
    flat[lone:lone + 32] = im.fake_sync(im.sync_params(every, 0), 1, 0x40)
    assert ((total + 15) // 16 + 4095) // 4096 == 4098 and total % 16 == 8
    cands = im.candidates(flat, total)
    ix = im.expect(flat, total, offs, lens, cands=cands)
    assert ix.n_found == 3 * 12 + 1 and ix.seg[12] is None and int(ix.cands[12]) == lone
    assert starts[1] < 4096 * 65536 < starts[1] + n and ix.streams[0].segments == 13
    _index_exact(hip, flat, offs, lens, ix=ix)


# ------------------------------------------------------------------------------------------------ capacity

def test_capacity_cut_on_and_beside_a_stream_boundary_and_a_tile_boundary(pkg, oracle):
    syn, hip = pkg.synth, pkg.hipdec
    cfg = syn.make_cfg(assignment=1, rate_code=0, n_aus=12, restart_interval=2)
    streams = [syn.stream(cfg, 7300 + i)[0] for i in range(30)]
    flat, offs, lens, total = im.lay_out(streams)
    assert 65536 < total <= 2 * 65536
    full = im.expect(flat, total, offs, lens)
    assert full.n_found == 180
    in_tile0 = int(np.searchsorted(full.cands, 65536))
    assert in_tile0 % 6 != 0                         # the tile boundary cuts a stream
    for ms in (59, 60, 61, 100, in_tile0 - 1, in_tile0, in_tile0 + 1, 180, 181):
        ix = im.expect(flat, total, offs, lens, max_segments=ms, cands=full.cands)
        assert ix.overflow == (ms < 180)
        behind = [x.capacity for x in ix.streams]
        assert behind == [ix.overflow and s >= (ms - 1) // 6 for s in range(30)]
        _index_exact(hip, flat, offs, lens, max_segments=ms, ix=ix)


# ------------------------------------------------------------------------------------------------ ranges

def test_ranges_of_2500_streams_are_checked_three_per_thread(pkg):
    syn, hip = pkg.synth, pkg.hipdec
    cfg = syn.make_cfg(assignment=1, rate_code=0, n_aus=2, restart_interval=1)
    base = [syn.stream(cfg, 7400 + i)[0] for i in range(4)]
    n = 2500
    flat, offs, lens, total = im.lay_out([base[i % 4] for i in range(n)])
    offs, lens = offs.astype(np.int64), lens.astype(np.int64)
    lens[0] += 1 << 40                                  # leaves the buffer
    offs[2] = offs[1]                                   # the same bytes twice
    offs[3] += 2                                        # misaligned
    lens[3] -= 2
    offs[1023] = offs[1000]                             # descending
    offs[1024] = 1 << 40                                # starts 2^40 behind the buffer
    offs[2499] = offs[2498]
    offs[1500] = offs[1499] + 16                        # starts inside the stream in front of it and ends in the one
    lens[1500] = 1300                                   # behind it: refused, and 1501 behind it too
    assert offs[1501] < offs[1500] + lens[1500] < offs[1502]
    soff, slen, refused = im.check_ranges(offs, lens, total)
    assert [i for i in range(n) if refused[i]] == [0, 2, 3, 1023, 1024, 1500, 1501, 2499]
    ix = im.expect(flat, total, offs, lens)
    ok = [x for x in ix.streams if not x.refused]
    assert all(x.resolvable and x.mlp_frames == 2 and x.segments == 2 and x.status == 0 for x in ok)
    bad = [x for x in ix.streams if x.refused]
    assert all((x.status, x.mlp_frames, x.segments) == (im.IRREGULAR | im.ENVELOPE, 0, 0) for x in bad)
    near = {i for r in (0, 2, 3, 1023, 1024, 1500, 1501, 2499) for i in range(2 * r - 3, 2 * r + 5) if 0 <= i < ix.n_found}
    _index_exact(hip, flat, offs, lens, sample=sorted(near), ix=ix)


# ------------------------------------------------------------------------------------------------ lane packing

@pytest.mark.parametrize("n", [2600, 4300])
def test_lane_packing_is_a_permutation_of_shuffled_shapes(pkg, oracle, n):
    """streams of 48 shape keys (1 - 8 units in the first segment x 2 rates x 3 assignments) in shuffled order, more
    than 4 MiB of them so that the packing runs (4300: the scan of the sorted counts in its multi-block form), on
    the lane kernels, interleaved, twice on one context"""
    syn, hip = pkg.synth, pkg.hipdec
    shapes = [(k, rate, a) for k in range(1, 9) for rate in (0, 1) for a in (1, 3, 12)]
    made = []
    for i, (k, rate, a) in enumerate(shapes):
        b = syn.stream(syn.make_cfg(assignment=a, rate_code=rate, n_aus=2 * k, restart_interval=k), 7500 + i)[0]
        made.append((b, syn.channels(a), rate))
    order = np.random.RandomState(77).randint(0, len(shapes), n)
    for edge in (256, 1024, 2048):
        assert set(order[edge - 128:edge]) & set(order[edge:edge + 128])        # equal keys on both sides
    flat, offs, lens, total = im.lay_out([made[j][0] for j in order])
    assert total > 4096 * 1024
    one = [im.single(b) for b, _, _ in made]
    assert all(x.resolvable and x.status == 0 and len(x.live) == 2 and x.live[0].nframes == k
               for x, (k, _, _) in zip(one, shapes))
    cache = {"key": order.tolist()}
    batch = hip.Batch(packed=(flat, offs, lens))
    ctx = hip.Context(0, n, 2 * n + 100, 3, hip.PCM_INTERLEAVED)
    try:
        for _ in range(2):
            pcm, infos, _ = hip.decode_batch(ctx, batch, hip.PCM_INTERLEAVED)
            assert ctx.segment_count() == 2 * n
            for s, (j, inf, got) in enumerate(zip(order.tolist(), infos, pcm)):
                b, nch, rate = made[j]
                if j not in cache:
                    cache[j] = oracle.decode(b, nch, (one[j].mlp_frames + 2) * im.ROWS_PER_AU[rate])
                w, r, st = cache[j]
                assert st == 0 and r == one[j].mlp_frames * im.ROWS_PER_AU[rate]
                assert inf.status & ~hip.ST_BENIGN == 0 and int(inf.pcm_frames) == r, "stream %d: %#x" % (s, inf.status)
                assert (int(inf.mlp_frames), int(inf.bytes_consumed), int(inf.segments)) == (
                    one[j].mlp_frames, one[j].bytes_consumed, 2), "stream %d" % s
                assert got.shape == w.shape and np.array_equal(got, w), "stream %d (shape %r): PCM differs" % (s, shapes[j])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the graph

@pytest.mark.parametrize("forked", [False, True])
def test_index_replayed_as_a_graph_on_buffers_overwritten_in_place(pkg, oracle, forked):
    """One Batch on a real stream, its bytes, offsets and lengths overwritten in place with two contents of the same
    total and stream count in turn: the index's launches are noted, captured and replayed (state 1, 2, 2); a call with
    another total resets the key.  Below 4 MiB the graph is linear, above it the lane packing forks a side stream."""
    import torch
    syn, hip = pkg.synth, pkg.hipdec
    n, slot = 24, 32768
    a = [syn.stream(syn.make_cfg(assignment=1, rate_code=0, n_aus=12, restart_interval=4), 7600 + i)[0] for i in range(n)]
    kinds = [(1, 0, 12, 2), (12, 1, 8, 1), (3, 0, 10, 5)]
    b = [syn.stream(syn.make_cfg(assignment=k[0], rate_code=k[1], n_aus=k[2], restart_interval=k[3]), 7700 + i)[0]
         for i, k in ((i, kinds[i % 3]) for i in range(n))]
    nch = {0: [2] * n, 1: [syn.channels(kinds[i % 3][0]) for i in range(n)]}
    rates = {0: [0] * n, 1: [kinds[i % 3][1] for i in range(n)]}
    total = n * slot + (4096 * 1024 if forked else 0)           # nobody's zero bytes behind the streams
    starts = [i * slot for i in range(n)]
    content = [im.lay_out(s, starts, total=total) for s in (a, b)]
    model = [im.expect(f, total, o, l) for f, o, l, _ in content]
    assert model[0].n_found != model[1].n_found and all(x.resolvable for m in model for x in m.streams)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    states = []
    with torch.cuda.stream(st):
        batch = hip.Batch(packed=content[0][:3])
        ctx = hip.Context(0, n, 1024)
        try:
            def round_(which):
                flat, offs, lens, _ = content[which]
                batch.d_bytes.copy_(torch.from_numpy(flat))
                batch.d_off.copy_(torch.from_numpy(offs.astype(np.int64)))
                batch.d_len.copy_(torch.from_numpy(lens.astype(np.int64)))
                ctx.index_batch(batch, st.cuda_stream)
                states.append(ctx.index_graph_state())
                im.compare(model[which], ctx.stream_info(stream=st.cuda_stream))
                assert ctx.segment_count(st.cuda_stream) == model[which].n_found
                _decode_against_oracle(hip, oracle, batch, offs, lens, nch[which], rates[which], model[which], ctx=ctx,
                                       stream=st.cuda_stream, cache=caches[which])
                states.append(ctx.index_graph_state())      # (decode_batch indexed once more)

            caches = [{"key": [("a", i) for i in range(n)]}, {"key": [("b", i) for i in range(n)]}]
            hosts = [c[0] for c in content]
            # the oracle's side once per content
            for which in (0, 1):
                flat, offs, lens, _ = content[which]
                for i in range(n):
                    s = flat[int(offs[i]):int(offs[i]) + int(lens[i])]
                    caches[which][caches[which]["key"][i]] = oracle.decode(
                        s, nch[which][i], (model[which].streams[i].mlp_frames + 2) * im.ROWS_PER_AU[rates[which][i]])
            for which in (0, 1, 0):
                round_(which)
            print("graph states, rounds 1-3:", states)
            assert states[0] == 1 and states[2:] == [2] * (len(states) - 2), states
            # another total: the key resets, the launches are direct
            ctx.index(batch.d_bytes.data_ptr(), total - 4096, batch.d_off.data_ptr(), batch.d_len.data_ptr(), n, st.cuda_stream)
            assert ctx.index_graph_state() == 1
            im.compare(im.expect(hosts[0][:total - 4096 + 64], total - 4096, content[0][1], content[0][2]),
                       ctx.stream_info(stream=st.cuda_stream))
            del states[:]
            for which in (1, 0, 1):
                round_(which)
            print("graph states, rounds 4-6:", states)
            assert states[0] == 1 and states[2:] == [2] * (len(states) - 2), states
        finally:
            st.synchronize()
            ctx.close()


# ------------------------------------------------------------------------------------------------ k_au_check

def _phased_units(stream):
    """units 1 .. 8 of `stream` moved to phases 2, 4, .., 14, 0 of a 16-byte chunk by zero bytes behind the unit in
    front of each"""
    out = stream
    for k in range(1, 9):
        at = im.unit_offsets(out)[k]
        grow = (2 * k - at) % 16
        if grow:
            out = stream_tools.padded_unit(out, k - 1, im.unit_size(out, im.unit_offsets(out)[k - 1]) + grow)
    assert [p % 16 for p in im.unit_offsets(out)[:9]] == [0, 2, 4, 6, 8, 10, 12, 14, 0]
    return out


def _substreams(b, unit, S):
    """[(first data byte, parity byte, CRC byte)] of the substreams of the access unit at offset `unit`
    (src/mlp.c:656-668: the info words behind the major sync, if any; extents in bytes from the end of the infos)"""
    pos = unit + (32 if stream_tools.is_major_sync(b, unit) else 4)
    ends, p = [], pos
    for _ in range(S):
        w = (int(b[p]) << 8) | int(b[p + 1])
        assert w & 0x2000, "the generator writes check bytes"
        ends.append(2 * (w & 0xFFF))
        p += 4 if w & 0x8000 else 2
    lo, out = 0, []
    for e in ends:
        out.append((p + lo, p + e - 2, p + e - 1))
        lo = e
    return out


SITES = ("first", "head", "tail", "last", "run-1", "run", "parity", "crc")


def _damage_at(b, unit, S, site, turn):
    """-> the byte to flip a bit in, for one site of a substream of the unit (turn picks the substream), or None"""
    subs = _substreams(b, unit, S)
    if site in ("run-1", "run"):
        for lo, par, _ in subs[turn % S:] + subs[:turn % S]:
            edge = (lo + 16 + 127) & ~127           # (streams are laid out at multiples of 128)
            if edge + 16 < par - 3:
                return edge - 1 if site == "run-1" else edge
        return None
    lo, par, crc = subs[turn % S]
    assert par - lo >= 40
    return {"first": lo, "head": lo + 1, "tail": par - 3, "last": par - 1, "parity": par, "crc": crc}[site]


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("assignment,rate", [(1, 0), (12, 1), (12, 2)])
def test_substream_checks_by_position(pkg, oracle, assignment, rate, S):
    """k_au_check is byte-parallel with ragged ends: substreams at all eight phases of a chunk, clean, and with one
    bit flipped per stream at every site of its arithmetic -- first and last data byte, the ragged head and tail chunk,
    both sides of a lane's 128-byte run, the parity byte, the CRC byte"""
    syn, hip = pkg.synth, pkg.hipdec
    nch, rows = syn.channels(assignment), im.ROWS_PER_AU[rate]
    cfg = syn.make_cfg(assignment=assignment, rate_code=rate, n_substreams=S, n_aus=10, restart_interval=4)
    good = _phased_units(syn.stream(cfg, 7800 + S)[0])
    units = im.unit_offsets(good)
    if rate == 2:
        assert max(par - lo for u in units for lo, par, _ in _substreams(good, u, S)) > 1024    # more than one 64-chunk pass
    streams, where = [good], [None]
    for k in range(8):
        for t, site in enumerate(SITES):
            at = _damage_at(good, units[k], S, site, k + t)
            if at is None:
                continue
            bad = good.copy()
            bad[at] ^= 0x10
            streams.append(bad)
            where.append((k, site))
    assert len(streams) > 1 + 8 * 6 and {"run-1", "run"} <= {w[1] for w in where[1:]}
    stride = (len(good) + 127) & ~127
    flat, offs, lens, total = im.lay_out(streams, [i * stride for i in range(len(streams))])
    batch = hip.Batch(packed=(flat, offs, lens))
    ctx = hip.Context(0, len(streams), 4 * len(streams))
    cap = 10 * rows
    out = hip.PcmRegions([cap] * len(streams), [nch] * len(streams))
    try:
        ctx.index_batch(batch)
        ctx.decode(*out.ptrs, 0)
        infos = ctx.stream_info()
        host = out.d_pcm.cpu().numpy().reshape(len(streams), nch, cap)
    finally:
        ctx.close()
    want, r, st = oracle.decode(good, nch, cap)
    assert st == 0 and r == cap
    assert infos[0].status & ~hip.ST_BENIGN == 0 and int(infos[0].pcm_frames) == cap and np.array_equal(host[0], want)
    both = hip.ST["PARITY"] | hip.ST["CRC"]
    wrong = []
    for i in range(1, len(streams)):
        k, site = where[i]
        w, r, st = oracle.decode(streams[i], nch, cap)
        got = int(infos[i].status)
        line = "unit %d %-6s oracle %#x (%d frames)  gpu %#x (%d frames)" % (k, site, st, r, got, infos[i].pcm_frames)
        print(line)
        assert st != 0                                                      # (the damage is one: the test's own premise)
        ok = bool(got & ~hip.ST_BENIGN)
        if st & both:
            ok = ok and bool(got & both) and (st & both == both or got & both == st & both)
        if not ok:
            wrong.append(line)
        elif not np.array_equal(host[i][:, :k * rows], want[:, :k * rows]):
            wrong.append(line + ": PCM in front of the unit differs")
    assert not wrong, "%d of %d damaged streams:\n%s" % (len(wrong), len(streams) - 1, "\n".join(wrong))
