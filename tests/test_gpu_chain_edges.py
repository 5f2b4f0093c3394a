"""The chain passes at the shapes where their pipelines turn (csrc/mlp_chain.h, csrc/mlp_chain_small.h): the table of
tests/chain_cases.py -- segment lengths round the unit ring and the turn, blocks that start at every frame of a unit and
one per unit, segments past the stamp wrap and past one rematrix step, chains of one-unit segments round the record ring,
batches of 1, 7, 8, 9 and 17 titles of unequal length with a long chain and a dead segment among them, regions that are
misaligned and capacities that end inside a unit -- through BOTH forms (hip.CHAIN_FORM 1: k_chain_fused, 2: k_chain_filter
+ k_chain_rematrix), each bit for bit against the oracle: PCM in both int32 layouts and as both WAV payloads, frame counts,
status, and per segment that the chain passes decoded it (DVDA_ST_CHAINED | DVDA_ST_GENERAL; never _SEQ, _TIMING or
_CAPACITY -- a _CAPACITY there is a record walk that overran).  tests/test_chain_model.py holds the premises without a
GPU: that the shapes are what the names say, and which segments continue a history.

Every buffer is filled with a sentinel first; nothing outside the regions (for a WAV payload: outside the valid bytes)
may change.  A region too small for its title: DVDA_ST_OVERFLOW, pcm_frames the size needed, the neighbour exact, a
second decode of the same index at that size exact; what the short region itself holds is not promised
(include/dvda_mlp_hip.h) and not looked at."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests.test_gpu_chain_forms import form          # noqa: F401  (the fixture: each form forced in turn)

pytestmark = pytest.mark.gpu

GUARD_WORDS = 64
INT32_LAYOUTS = ("planar", "interleaved")
ALL_LAYOUTS = INT32_LAYOUTS + ("wav16", "wav24")


def _lay(hip, layout):
    return {"planar": hip.PCM_PLANAR, "interleaved": hip.PCM_INTERLEAVED, "wav16": hip.PCM_WAV16,
            "wav24": hip.PCM_WAV24}[layout]


def _place(hip, rows, chans, lay, mis):
    """-> (out_off[i], words of the buffer): region i starts mis[i] words behind a 16-byte boundary, GUARD_WORDS sentinel
    words in front of the first, between neighbours and behind the last"""
    off, pos = [], GUARD_WORDS
    for r, c, m in zip(rows, chans, mis):
        pos = ((pos + 3) & ~3) + m
        off.append(pos)
        pos += hip.region_words(r, c, lay) + GUARD_WORDS
    return off, pos


def _decode(hip, ctx, rows, chans, lay, mis=None):
    """one decode of ctx's index into fresh sentinel-filled regions -> (infos, host copy of the buffer, out_off); nothing
    outside the regions' valid bytes may have changed"""
    n = len(rows)
    out_off, words = _place(hip, rows, chans, lay, mis or [0] * n)
    last = max(o + hip.region_words(r, c, lay) for o, r, c in zip(out_off, rows, chans))
    out = hip.PcmRegions(rows, chans, lay, out_off=out_off, slack=words - last, fill=cc.SENTINEL)
    assert out.d_pcm.numel() == words
    ctx.decode(*out.ptrs, 0)
    infos = list(ctx.stream_info(n))
    host = out.d_pcm.cpu().numpy()
    by = host.view(np.uint8)
    outside = np.ones(len(by), bool)
    nb = hip.sample_bytes(lay)
    for o, r, c in zip(out_off, rows, chans):
        outside[4 * o:4 * o + r * c * nb] = False
    assert outside.sum() >= 4 * GUARD_WORDS * (n + 1)
    bad = np.flatnonzero(outside & (by != (cc.SENTINEL & 0xFF)))
    assert bad.size == 0, "stray stores at bytes %s (regions at words %s)" % (bad[:8].tolist(), out_off)
    return infos, host, out_off


def _exact(hip, oracle, cases, infos, host, out_off, rows, lay, which=None):
    """titles `which` (default: all) are what the oracle says: status, frames, every value or payload byte"""
    chans = [c.nch for c in cases]
    got = hip.cut_regions(host, out_off, rows, chans, [inf.pcm_frames for inf in infos], lay)
    for i, (c, g, inf) in enumerate(zip(cases, got, infos)):
        if which is not None and i not in which:
            continue
        want, r, st = cc.oracle_pcm(oracle, c)
        assert st == 0
        assert inf.status & ~hip.ST_BENIGN == 0, "%s: status %#x" % (c.name, inf.status)
        assert inf.pcm_frames == r and inf.channels == c.nch, (c.name, inf.pcm_frames, r)
        if hip.sample_bytes(lay) != 4:
            ref = np.frombuffer(oracle.wav_pack(want, 8 * hip.sample_bytes(lay)), np.uint8)
            assert len(g) == len(ref) and np.array_equal(g, ref), "%s: first difference at byte %d" % (
                c.name, int(np.argmax(g != ref)) if len(g) == len(ref) else -1)
        else:
            assert g.shape == want.shape
            assert np.array_equal(g, want), "%s differs at %s" % (c.name, np.argwhere(g != want)[:4].tolist())


SEG_BITS = ("CHAINED", "GENERAL", "SEQ", "TIMING", "CAPACITY")


def _segments(hip, ctx, n_streams):
    """the live segments of every stream, in stream order (retired sync candidates left out)"""
    per = [[] for _ in range(n_streams)]
    for j in range(ctx.segment_count()):
        s = ctx.segment_info(j)
        if not s.status & hip.ST["FALSE_SYNC"]:
            per[s.stream].append((int(s.offset), int(s.status)))
    return [[st for _, st in sorted(p)] for p in per]


def _decoded_by_the_chain_passes(hip, oracle, cases, segs):
    """every segment that continues a history (chain_cases.history_matters) carries CHAINED | GENERAL, and no segment
    SEQ, TIMING, CAPACITY or an error"""
    ST = hip.ST
    both = ST["CHAINED"] | ST["GENERAL"]
    for c, mine in zip(cases, segs):
        m = cc.history_matters(oracle, c)
        assert len(mine) == len(m), (c.name, len(mine), len(m))
        for k, (st, needs) in enumerate(zip(mine, m)):
            assert st & ~hip.ST_BENIGN == 0 and st & (ST["SEQ"] | ST["TIMING"] | ST["CAPACITY"]) == 0, (c.name, k, hex(st))
            if needs:
                assert st & both == both, "%s segment %d: status %#x" % (c.name, k, st)


def _named(hip, st):
    return "|".join(b for b in SEG_BITS if st & hip.ST[b]) or "0"


def _run(pkg, oracle, names, lanes, layouts=INT32_LAYOUTS, max_segments=1024):
    """the titles `names` as one batch, once per layout: exact, and decoded by the chain passes -> the segments' status
    words of the last layout"""
    hip = pkg.hipdec
    cases = [cc.case(pkg.synth, n) for n in names]
    batch = hip.Batch([c.data for c in cases])
    rows, chans = [c.frames for c in cases], [c.nch for c in cases]
    segs = None
    for layout in layouts:
        lay = _lay(hip, layout)
        ctx = hip.Context(0, len(cases), max_segments, lanes, lay)
        try:
            ctx.index_batch(batch)
            infos, host, out_off = _decode(hip, ctx, rows, chans, lay)
            segs = _segments(hip, ctx, len(cases))
        finally:
            ctx.close()
        _exact(hip, oracle, cases, infos, host, out_off, rows, lay)
        if names != ["iir_96k"]:
            _decoded_by_the_chain_passes(hip, oracle, cases, segs)
    return segs


# ------------------------------------------------------------------------------------- segment lengths, block starts
@pytest.mark.parametrize("lanes", [0, 2, 64])
@pytest.mark.parametrize("name", [n for n in cc.SEG_LEN + cc.BLOCKS if n != "iir_96k"])
def test_segment_lengths_and_block_starts(pkg, oracle, form, name, lanes):
    _run(pkg, oracle, [name], lanes)


@pytest.mark.parametrize("lanes", [0, 2, 64])
def test_iir_segments_go_where_the_table_says(pkg, oracle, form, lanes):
    """IIR | CHAINED: exact like the others, and its segments behind the first end up where chain_cases.IIR_SEGMENTS
    records -- decoded by the chain passes' frame-by-frame path (seg_meta bit 9), not handed to the sequential pass"""
    hip = pkg.hipdec
    segs = _run(pkg, oracle, ["iir_96k"], lanes)[0]
    got = [_named(hip, st) for st in segs[1:]]
    print("iir_96k form %d lanes %d: %s" % (form, lanes, got))
    assert got == cc.IIR_SEGMENTS


# ------------------------------------------------------------------------------------------------------- the batches
@pytest.mark.parametrize("batch", list(cc.BATCHES))
def test_batches_of_unequal_chains(pkg, oracle, form, batch):
    """every title of the batch exact (lanes_per_segment rotates over the batches)"""
    names = cc.BATCHES[batch]
    _run(pkg, oracle, names, cc.lanes_for(list(cc.BATCHES).index(batch)))


# ------------------------------------------------------------------------------------------------------------ output
def _output_batch(pkg, name):
    """the title under test and a neighbour in the same batch (another output row of the other channel count)"""
    other = {"out_seg15_6ch": "out_blk5_2ch", "out_seg15_2ch": "out_blk5_6ch", "out_blk5_6ch": "out_seg15_2ch",
             "out_blk5_2ch": "out_seg15_6ch"}[name]
    return [cc.case(pkg.synth, name), cc.case(pkg.synth, other)]


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("name", cc.OUTPUT)
def test_misaligned_regions_and_short_capacities(pkg, oracle, form, name, layout):
    """ONE index, decoded into regions 1, 2 and 3 words off a 16-byte boundary at every capacity of chain_cases.CAPACITIES:
    full -- exact, decoded by the chain passes --; short -- DVDA_ST_OVERFLOW and the size needed, the neighbour exact,
    then the same index again at the reported size, exact.  The guards hold every time, to the byte.
    (Capacity "1" ends inside the title's first segment, the fast pass's: with the lane kernels -- lanes_per_segment 2,
    which the rotation gives five of the sixteen cases -- that lane stops there and leaves no FIR history, and the chain
    behind it used to report DVDA_ST_ENVELOPE, from the fused form DVDA_ST_CAPACITY too, and too few pcm_frames.)"""
    hip = pkg.hipdec
    lay = _lay(hip, layout)
    cases = _output_batch(pkg, name)
    full = cases[0].frames
    chans = [c.nch for c in cases]
    lanes = cc.lanes_for(cc.OUTPUT.index(name) + ALL_LAYOUTS.index(layout))
    batch = hip.Batch([c.data for c in cases])
    ctx = hip.Context(0, 2, 1024, lanes, lay)
    try:
        ctx.index_batch(batch)
        for mis in cc.MISALIGN:
            for which in cc.CAPACITIES:
                cap = cc.capacity(which, full)
                assert 1 <= cap <= full
                rows = [cap, cases[1].frames]
                infos, host, out_off = _decode(hip, ctx, rows, chans, lay, [mis, (mis + 1) & 3])
                if cap == full:
                    _exact(hip, oracle, cases, infos, host, out_off, rows, lay)
                    _decoded_by_the_chain_passes(hip, oracle, cases, _segments(hip, ctx, 2))
                    continue
                st = infos[0].status
                assert st & hip.ST["OVERFLOW"] and st & ~(hip.ST_BENIGN | hip.ST["OVERFLOW"]) == 0, (which, mis, hex(st))
                assert infos[0].pcm_frames == full, (which, mis, infos[0].pcm_frames)
                _exact(hip, oracle, cases, infos, host, out_off, rows, lay, which={1})
                rows = [int(infos[0].pcm_frames), cases[1].frames]
                infos, host, out_off = _decode(hip, ctx, rows, chans, lay, [mis, (mis + 1) & 3])
                _exact(hip, oracle, cases, infos, host, out_off, rows, lay)
    finally:
        ctx.close()
