"""Chain passes, CPU side: the premises of tests/test_gpu_chain_edges.py, held on the oracle and on the bytes, so that the
GPU file cannot pass for a reason other than the one it is written for -- every stream of tests/chain_cases.py decodes
clean and is what the compiled reference makes of it, the shapes are what the rows' names say (segment lengths from the
major syncs in the bytes, block starts by the generator's rule), each of the eight code paths the table is there for has
rows that reach it, the FIR history a chain carries from segment to segment changes the PCM, and the constants the shapes
are derived from are the ones the headers state."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests import oracle_lib
from tests.stream_tools import frame_offsets, major_syncs

NAMES = list(cc.ROWS)
CHAINED_ROWS = [n for n in NAMES if len(cc.segment_aus(cc.ROWS[n])) > 1]


def test_constants_are_the_headers(pkg):
    """a changed constant fails here instead of silently moving the edges away from the table"""
    want = dict(UNIT=cc.UNIT, FU_T=cc.FU_T, FU_DT=cc.FU_DT, FU_RING=cc.FU_RING, FU_RECS=cc.FU_RECS, FU_BRECS=cc.FU_BRECS,
                GROUP_CHAINS=cc.GROUP_CHAINS, CHAIN_BUCKETS=cc.CHAIN_BUCKETS, BUCKET_FRAMES=cc.BUCKET_FRAMES,
                CHAIN_DEPTH=cc.CHAIN_DEPTH, REMAT_FRAMES=cc.REMAT_FRAMES, REMAT_STEP=cc.REMAT_STEP,
                STAMP_TURNS=cc.STAMP_TURNS)
    assert cc.header_constants() == want
    assert cc.RPA == {r: pkg.synth.rows_per_au(r) for r in (0, 1, 2)}
    assert all(v % cc.UNIT == 0 for v in cc.RPA.values())


@pytest.mark.parametrize("name", NAMES)
def test_stream_decodes_clean_and_as_the_reference(pkg, oracle, name):
    c = cc.case(pkg.synth, name)
    pcm, r, st = cc.oracle_pcm(oracle, c)
    assert st == 0 and r == c.frames == c.row.n_aus * c.rpa and pcm.shape == (c.nch, r)
    assert pcm.any(axis=1).all()                                # no channel is silence
    assert len(c.data) < 1 << 20
    assert oracle_lib.same_as_reference(
        "chain_%s" % name, (pcm, r),
        lambda: oracle_lib.Reference().decode(c.data, c.cfg.assignment, c.cfg.rate_code, c.cfg.bps_code, r))


@pytest.mark.parametrize("name", NAMES)
def test_segments_are_what_the_row_says(pkg, name):
    """from the bytes: a major sync at every `interval`-th access unit and nowhere else"""
    c = cc.case(pkg.synth, name)
    offs, syncs = frame_offsets(c.data), major_syncs(c.data)
    assert len(offs) == c.row.n_aus and offs[-1] + 2 * (((int(c.data[offs[-1]]) & 0xF) << 8) | int(c.data[offs[-1] + 1])) == len(c.data)
    at = [offs.index(p) for p in syncs]
    assert at == list(range(0, c.row.n_aus, c.row.interval))
    assert np.diff(at + [len(offs)]).tolist() == cc.segment_aus(c.row)
    assert (int(c.data[20]) >> 4) == c.row.S
    if c.row.false_sync is not None:
        # the planted header: in the ignored tail of its unit, in a segment behind the first, not the chain's last
        u = c.row.false_sync
        end = offs[u + 1]
        assert bytes(c.data[end - 64 + 4:end - 64 + 8]) == b"\xF8\x72\x6F\xBB"
        seg = u // c.row.interval
        assert 1 <= seg < len(syncs) - 1


def test_block_starts_reach_every_residue():
    """split_rows' rule (chain_cases.block_starts): over the DISC rows of the blocks group a block starts at every frame
    of a unit, 0 .. 7 -- and the 8-frame-block stream has a block, so a block record, per unit"""
    res = set()
    for name in cc.BLOCKS:
        r = cc.ROWS[name]
        if "DISC" in r.feats:
            starts = cc.block_starts(r)
            assert len(starts) == r.blocks <= 8
            res |= {s % cc.UNIT for s in starts}
    assert res == set(range(cc.UNIT))
    assert cc.block_starts(cc.ROWS["blk3_48k"]) == [0, 13, 26]
    assert cc.block_starts(cc.ROWS["blk4_48k"]) == [0, 10, 20, 30]
    assert cc.block_starts(cc.ROWS["blk7_96k"]) == [0, 11, 22, 33, 44, 55, 66]
    assert {s % 8 for s in cc.block_starts(cc.ROWS["blk7_96k"])[1:]} == {3, 6, 1, 4, 7, 2}
    assert cc.block_starts(cc.ROWS["blk8_96k"]) == list(range(0, 80, 10))
    assert cc.block_starts(cc.ROWS["blk8_192k"]) == list(range(0, 160, 20))
    for name in ("blk5_48k", "out_blk5_2ch"):
        r = cc.ROWS[name]
        assert cc.block_starts(r) == list(range(0, cc.RPA[r.rate], cc.UNIT))
        for n_au in cc.segment_aus(r)[1:]:                      # exactly R / 8 blocks per segment: rmax = R / 8 + 1 is full
            R = n_au * cc.RPA[r.rate]
            assert n_au * len(cc.block_starts(r)) == R // cc.UNIT
            assert R // cc.UNIT >= cc.FU_BRECS                  # ... and more records than the lane's ring holds


def test_iir_and_varblock_rows_hold_what_they_name(pkg, oracle):
    for name in cc.BLOCKS:
        c = cc.case(pkg.synth, name)
        _, _, st, stats = oracle.decode_stats(c.data, c.nch, c.frames)
        assert st == 0
        assert (sum(stats.iir_order[1:]) > 0) == (name == "iir_96k"), name
    assert "VARBLOCK" in cc.ROWS["varblock_96k"].feats


def test_segment_lengths_cover_the_edges():
    """of the segments the chain passes decode (behind each title's first)"""
    units = sorted({u for n in cc.SEG_LEN for u in cc.chained_units(cc.ROWS[n])})
    assert units[0] == 5
    assert any(u < cc.FU_RING for u in units)
    assert any(cc.FU_RING <= u <= cc.FU_RING + cc.FU_T for u in units) and 15 in units
    assert any(u % cc.FU_T for u in units) and any(u % cc.FU_T == 0 for u in units)
    assert {5, 10, 15, 20, 35} <= set(units)
    assert any(u > cc.STAMP_TURNS * cc.FU_T for u in units)                             # the turn stamps wrap
    frames = [u * cc.UNIT for u in units]
    assert 10240 in frames and 4400 in frames
    assert sorted({-(-f // cc.REMAT_STEP) for f in frames}) == [1, 2, 3]                 # remat_blocks
    assert 4400 % cc.REMAT_FRAMES == 48                                                 # a last rematrix block of 48 frames
    # a segment that ends within FU_DT + 1 turns of its set-up
    assert any(-(-u // cc.FU_T) <= cc.FU_DT + 1 for u in units)
    # one-unit segments: a chain of them goes more than three times round the record ring
    for name in ("seg5_48k", "seg10_96k", "seg20_192k"):
        n = cc.chained_units(cc.ROWS[name])
        assert len(n) >= 24 > 3 * cc.FU_RECS - 1 and len(n) > 3 * cc.FU_RECS - 1
        assert len(set(n)) == 1
    # the rows kept as the issue states them are one segment, the fast pass's: nothing for the chain passes
    assert cc.chained_units(cc.ROWS["seg1280_192k"]) == [] and cc.chained_units(cc.ROWS["seg4400f_48k"]) == []


def test_batches_are_made_up_as_named(pkg, oracle):
    g = cc.GROUP_CHAINS
    assert cc.BATCH_SIZES == (1, g - 1, g, g + 1, 2 * g + 1)
    aus = [cc.ROWS[t].n_aus for t in cc.BATCHES["batch17"]]
    assert min(aus) == 1 and max(aus) == 40 and len(set(aus)) == 17
    assert cc.chain_frames(cc.ROWS["t01"]) == 0                                          # a title with no chain at all
    assert cc.chain_frames(cc.ROWS["t00"]) > 0                                           # (the batch of one has one)
    for name, titles in cc.BATCHES.items():
        rows = [cc.ROWS[t] for t in titles]
        # (the chains as the history makes them: runs of segments that each continue the one before)
        chains = [f for t in titles for f in cc.chains(oracle, cc.case(pkg.synth, t))]
        assert len(chains) >= len(titles) - 1
        classes = {min(f // cc.BUCKET_FRAMES, cc.CHAIN_BUCKETS) for f in chains}
        if len(titles) >= g - 1:
            assert len(classes) >= 4, (name, sorted(classes))
            assert {r.S for r in rows} == {1, 2} and {r.asg for r in rows} == {12, 1, 0x12}
            assert {r.rate for r in rows} == {0, 1, 2}
            # chains of very unequal length side by side: the shortest ends many turns before the longest
            assert max(chains) >= 20 * min(chains)
            assert any(r.false_sync is not None for r in rows)
        long_ones = [f for f in chains if f > cc.CHAIN_BUCKETS * cc.BUCKET_FRAMES]
        assert len(long_ones) == (1 if "long" in name else 0)
    assert cc.ROWS["long_s1"].S == 1 and cc.ROWS["long_s2"].S == 2
    assert cc.chain_frames(cc.ROWS["long_s1"]) == 65920 > 65536


def test_every_path_has_its_rows():
    """which row reaches which of the eight shapes chain_cases.PATHS lists -- the premise of each, from the rows"""
    by_path = {p: [n for n, r in cc.ROWS.items() if p in r.paths] for p in cc.PATHS}
    assert all(by_path[p] for p in cc.PATHS), by_path
    for n in by_path[1]:
        assert min(cc.chained_units(cc.ROWS[n])) < cc.FU_RING
    for n in by_path[2]:
        assert any(u % cc.FU_T for u in cc.chained_units(cc.ROWS[n]))
    for n in by_path[3]:
        assert "DISC" in cc.ROWS[n].feats and np.diff(cc.block_starts(cc.ROWS[n])).tolist() == [cc.UNIT] * 4
    for n in by_path[4]:
        r = cc.ROWS[n]
        assert "VARBLOCK" in r.feats or ("DISC" in r.feats and any(s % cc.UNIT for s in cc.block_starts(r)))
    for n in by_path[5]:
        r = cc.ROWS[n]
        assert (max(cc.chained_units(r)) > cc.STAMP_TURNS * cc.FU_T or max(cc.chained_units(r)) * cc.UNIT > cc.REMAT_STEP or
                cc.chain_frames(r) > cc.CHAIN_BUCKETS * cc.BUCKET_FRAMES)
    for n in by_path[6]:
        r = cc.ROWS[n]
        assert r.interval == 1 and len(cc.chained_units(r)) > 3 * cc.FU_RECS - 1
    assert set(by_path[7]) == set(cc.TITLES) and set(by_path[8]) == set(cc.OUTPUT)
    assert {cc.ROWS[n].asg for n in cc.OUTPUT} == {12, 1}
    # every row with a chain is in a group the GPU file runs
    assert set(NAMES) == set(cc.SEG_LEN) | set(cc.BLOCKS) | set(cc.OUTPUT) | set(cc.TITLES)
    assert all(t in cc.ROWS for titles in cc.BATCHES.values() for t in titles)
    assert {t for titles in cc.BATCHES.values() for t in titles} == set(cc.TITLES)


@pytest.mark.parametrize("name", CHAINED_ROWS)
def test_history_in_front_of_the_chained_segments_matters(pkg, oracle, name):
    """The bytes of a segment behind the first, decoded alone -- that is: with a FIR history of zeros --, must not give
    the PCM of the whole decode (chain_cases.history_matters): then the segment's first block runs FIR taps on the
    history of the segment before it (DVDA_ST_CHAINED: the chain passes' to decode), and a chain pass that lost the
    history would not pass.  Held for EVERY segment behind the first of the seg_len, blocks and output rows and of the
    long titles (their seeds are chosen for it); the other titles may hold a segment that opens without taps -- the fast
    pass's, it cuts the title into two chains --, never only such."""
    c = cc.case(pkg.synth, name)
    m = cc.history_matters(oracle, c)
    assert len(m) == len(cc.segment_aus(c.row)) and not m[0]
    if c.row.group != "groups" or name.startswith("long"):
        assert all(m[1:]), (name, [k for k, v in enumerate(m) if k and not v])
    else:
        assert any(m[1:]), (name, m)


def test_the_titles_also_hold_a_chain_cut_in_two(pkg, oracle):
    """(what the generator's order-0 openings give for free: a title whose chain stops at a segment of the fast pass's
    and starts again behind it, from the history that segment's lane left)"""
    cut = [t for t in cc.BATCHES["batch17"] if not all(cc.history_matters(oracle, cc.case(pkg.synth, t))[1:])]
    assert cut and set(cut) & set(cc.BATCHES["batch7"])
