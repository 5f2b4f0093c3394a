"""The serial index model (tests/index_model.py) held to the oracle's framing, and its case builders held to the
positions and the class they aim at.  CPU only."""
import numpy as np
import pytest

from tests import index_model as im
from tests import stream_tools


@pytest.fixture(scope="module")
def cases(pkg):
    return im.benign_cases(pkg.synth)


def test_model_counts_what_the_oracle_decodes(pkg, oracle, cases):
    """every benign case: the oracle's PCM frame count is the model's mlp_frames times the rate's rows per access
    unit, and its SYNC_CHANGE bit the model's -- resolvable or not, the serial walk is the reference's"""
    assert len(cases) > 25
    for name, b, nch, rate, _ in cases:
        x = im.single(b)
        rows = im.ROWS_PER_AU[rate]
        pcm, r, st = oracle.decode(b, nch, (x.mlp_frames + 2) * rows)
        print("%-26s units %3d dropped %2d oracle frames %6d status %#x" % (
            name, x.mlp_frames, sum(g.ndrop for g in x.live), r, st))
        assert r == x.mlp_frames * rows, name
        assert bool(st & 2) == bool(x.status & im.SYNC_CHANGE), name
        assert x.bytes_consumed == sum(im.unit_size(b, p) for p in x.units)


def test_model_records_of_the_plain_cases(pkg, cases):
    by = {name: b for name, b, *_ in cases}
    clean = im.single(by["clean"])
    assert clean.status == 0 and clean.mlp_frames == 24 and clean.bytes_consumed == len(by["clean"])
    assert [g.nframes for g in clean.live] == [4] * 6 and clean.segments == 6
    for short in (1, 3, 4, 31, 33, 123):
        x = im.single(by["cut-%d" % short])
        assert x.status == im.TRUNCATED and x.mlp_frames < 24 and x.live[-1].flags == im.TRUNCATED
    x = im.single(by["cut-in-last-sync"])
    assert x.status == im.TRUNCATED and x.mlp_frames == 20 and x.segments == 5      # the cut sync: no candidate of the range
    x = im.single(by["changed-70-in-a-row"])
    assert x.status == im.SYNC_CHANGE and x.mlp_frames == 10 and x.live[1].ndrop == 70 and x.segments == 80
    x = im.single(by["own-false-64-unit-9"])
    assert x.status == 0 and x.mlp_frames == 24 and x.segments == 6 + 64
    x = im.single(by["false-past-the-end"])
    assert x.status == 0 and x.segments == 9


def test_builders_hit_what_they_aim_at(pkg, cases):
    by = {name: b for name, b, *_ in cases}
    assert [p % 16 for p in stream_tools.major_syncs(by["phases"])[:9]] == [0, 2, 4, 6, 8, 10, 12, 14, 0]
    # place_sync: the pattern bytes p + 4 .. p + 7 across the boundary B for every start B - 16 .. B
    every = by["every-unit-a-sync"]
    first = im.unit_size(every, 0)
    for B in (256 * ((first + 18 + 255) // 256), 16384, 65536):
        for t in range(B - 16, B + 2, 2):
            base = im.start_for(t, first)
            s = im.place_sync(every, base, 1, t)
            assert base % 16 == 0 and base + stream_tools.major_syncs(s)[1] == t
            assert im.is_major_sync(s, t - base, len(s)) and im.single(s).mlp_frames == 80
        straddling = [t for t in range(B - 16, B + 2, 2) if t + 4 < B < t + 8]
        assert straddling == [B - 6]
    # the two classes
    assert all(im.single(b).resolvable == r for _, b, _, _, r in cases)
    x = im.single(by["own-false-200"])
    assert not x.resolvable and x.mlp_frames == 24 and x.status == 0        # benign for the reference all the same
    # candidates(): the array scan against the definition, offset by offset
    b = by["foreign-false-200"]
    flat, offs, lens, total = im.lay_out([b, by["clean"]])
    slow = [p for p in range(0, total - 31, 2) if im.is_major_sync(flat, p, total)]
    assert im.candidates(flat, total).tolist() == slow and len(slow) == 6 + 200 + 6


def test_check_ranges_serial_maximum():
    total = 4096
    offs = [0, 256, 256, 128, 1024, 1032, 2048, 1 << 41, 3072, 2560, 4096]
    lens = [256, 256, 16, 16, 512, 16, 1 << 40, 16, 1024, 16, 0]
    soff, slen, refused = im.check_ranges(offs, lens, total)
    assert refused == [False, False, True, True, False, True, True, True, False, True, False]
    assert slen == [256, 256, 0, 0, 512, 0, 0, 0, 1024, 0, 0]
    assert soff == sorted(soff) and max(soff) <= total
    # a range that leaves the buffer has no end (index 6 does not stand in the way of 8); one refused for its place
    # has: [0, 100), [48, 200) refused, [112, ..) refused behind it
    _, _, r = im.check_ranges([0, 48, 112, 208], [100, 152, 16, 16], total)
    assert r == [False, True, True, False]


def test_capacity_cut_in_the_model(pkg, cases):
    by = {name: b for name, b, *_ in cases}
    flat, offs, lens, total = im.lay_out([by["clean"]] * 3)
    full = im.expect(flat, total, offs, lens)
    assert full.n_found == 18 and not full.overflow
    for ms, behind in ((18, 3), (17, 2), (12, 1), (11, 1), (13, 2), (6, 0)):
        ix = im.expect(flat, total, offs, lens, max_segments=ms)
        assert ix.overflow == (ms < 18) and len(ix.cands) == ms
        assert [x.capacity for x in ix.streams] == [s >= behind for s in range(3)] or not ix.overflow
        for s in range(min(behind, 3)):
            assert ix.streams[s].mlp_frames == 24 and ix.streams[s].segments == 6
