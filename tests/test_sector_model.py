"""Sector tier, no GPU: the premises of tests/sector_cases.py asserted, its model against the muxer, and its model
against the REAL reference (oracle/_ref/dvda2wav_ref, or the stored digests of its output where it is not built).

Where the reference's reader and the device calls part ways -- stated here once, pinned on the GPU in
tests/test_gpu_sectors.py, not "fixed":
  * 1-5 stray bytes behind a sector's last packet: the reference stops reading the track there (src/packet.c:91-115),
    the kernels accept the sector;
  * a parameter block that differs from the track's: the reference ends the track (src/dvd-audio.c:1051-1056), the
    device call does not look at it;
  * a packet behind a track's first that completes no PCM frame (no whole chunk, no whole MLP access unit): dvda_read
    takes "0 frames" for the end of the stream (src/dvd-audio.c:767-775), the kernels go on.
test_reference_ends_a_track_where_the_kernels_go_on shows all three on two-sector tracks."""
import os
import tempfile

import numpy as np
import pytest

from tests import oracle_lib
from tests import sector_cases as sc
from tests.test_dvda2wav_e2e import REF_TOOL, _run

REF_LAYOUTS = [(16, 2, 1), (24, 1, 0), (24, 3, 2), (24, 5, 6), (24, 6, 12)]


def _chunk_offsets(sector, cs):
    why, pk = sc.walk(sector, 0xA0)
    assert why is None
    return [(off + t * cs, k, ln // cs) for k, (off, ln) in enumerate(pk) for t in range(ln // cs)], pk


# ------------------------------------------------------------------------------------------------ premises
@pytest.mark.parametrize("bps,ch,asg", sc.LAYOUTS)
def test_premise_the_old_shapes_reach_only_even_chunk_offsets(pkg, bps, ch, asg):
    """The gap, written down once: disc._sector puts the payload at 14 + 6 + 7 + 9 + an even fill, so every chunk
    offset of tests/test_pcm.py's sectors is even -- alignbyte shifts 1 and 3 never ran."""
    cs = 2 * ch * (bps // 8)
    s = np.zeros((5000 + 2 * ch, ch), np.int64)
    seen = set()
    for sec in pkg.disc.pcm_track_sectors(s, {16: 0, 24: 2}[bps], 1, asg):
        offs, pk = _chunk_offsets(sec, cs)
        assert len(pk) == 1
        seen |= {bo & 3 for bo, _, _ in offs}
    assert seen and seen <= {0, 2}


@pytest.mark.parametrize("bps,ch,asg", sc.LAYOUTS)
def test_premise_the_table_reaches_every_shift_count_and_edge(bps, ch, asg):
    cs = 2 * ch * (bps // 8)
    shifts, n_packets, n_chunks, starts_in_one = set(), set(), set(), set()
    ends_at_2047 = reads_extra_vector = False
    for name, sh in sc.SECTOR_SHAPES.items():
        sec, s, _ = sc.pcm_sector(sh, bps, ch, asg, 1)
        offs, pk = _chunk_offsets(sec, cs)
        shifts |= {bo & 3 for bo, _, _ in offs}
        n_packets.add(len(pk))
        n_chunks |= {ln // cs for _, ln in pk}
        starts_in_one.add(len({off & 3 for off, _ in pk}))
        ends_at_2047 |= any(off + ln == sc.SECTOR for off, ln in pk)
        # the funnel shift of a chunk's last dword reads word (bo >> 2) + ND: word 512 is the extra LDS vector
        reads_extra_vector |= any((bo >> 2) + (cs + 3) // 4 == 512 for bo, _, _ in offs)
    assert shifts == {0, 1, 2, 3}
    assert {1, 2, 3, 8} <= n_packets
    assert max(starts_in_one) >= 3                       # packets of one sector start at different off & 3
    most = (sc.SECTOR - 14 - 6 - 7 - 9) // cs
    assert {0, 1} <= n_chunks and max(n_chunks) == most
    if most >= 65:
        assert {63, 64, 65} <= n_chunks                  # the t += 64 lane loop: one turn, exactly one, two
    else:
        assert (bps, ch) == (24, 6) and most == 55       # 36-byte chunks: a packet never has 64
    assert ends_at_2047 and reads_extra_vector


def test_premise_remainders_are_dropped_per_packet():
    """src/pcm.c:147: two packets of 1.5 chunks hold 2 chunks, not 3"""
    sh = sc.shape([sc.A(("c", 1, 4)), sc.A(("c", 1, 4))])
    sec, s, _ = sc.pcm_sector(sh, 16, 2, 1)
    m = sc.model_pcm(np.frombuffer(sec, np.uint8), 16, 2)
    assert m.base[-1] == 4 and np.array_equal(m.pcm, s.T)


def _mlp_run():
    data = ((np.arange(40000) * 73 + 5) >> 2).astype(np.uint8)
    secs = sc.mlp_sectors(list(sc.MLP_SHAPES), data)
    return data, np.frombuffer(b"".join(secs), np.uint8)


def test_premise_the_mlp_table_reaches_every_alignment_and_length():
    data, sectors = _mlp_run()
    m = sc.model_mlp(sectors)
    assert m.bad == 0
    assert {d & 3 for d, ln, off in m.packets} == {0, 1, 2, 3}
    assert {(off & 3, d & 3) for d, ln, off in m.packets if ln >= 8} == {(a, b) for a in range(4) for b in range(4)}
    lens = {ln for d, ln, off in m.packets}
    assert set(range(8)) <= lens
    # shorter than the head run: the packet ends before the first aligned destination
    assert any(ln < ((4 - (d & 3)) & 3) for d, ln, off in m.packets)
    assert any(ln > 64 * 4 + 8 for d, ln, off in m.packets)          # the dword loop takes a second turn
    assert any(off + ln == sc.SECTOR for d, ln, off in m.packets)


@pytest.mark.parametrize("mlp", [False, True])
def test_premise_every_rejection_rule_is_reached_by_one_changed_field(mlp):
    want = 0xA1 if mlp else 0xA0
    params = b"" if mlp else sc.params_block(16, 1)
    for n in (1, 8):
        assert sc.walk(sc.good_base(params, want, n), want)[0] is None
    seen = []
    for rule in sc.rules_for(mlp):
        bad = sc.malformed(rule, mlp=mlp)
        assert sc.walk(bad, want)[0] == rule                         # that reason and no earlier one
        good = sc.good_base(params, want, 9 if rule == "ninth" else 1)
        if rule != "ninth":
            assert 1 <= sum(a != b for a, b in zip(bad, good)) <= 2, rule     # one field (a length is two bytes)
        seen.append(rule)
    assert len(seen) == (14 if mlp else 15)


@pytest.mark.parametrize("mlp", [False, True])
def test_premise_long_runs_put_every_rule_at_every_named_position(mlp):
    """over the cases of tests/test_gpu_sectors.py's sector-count tests (12 layouts; 14 shifts for the demux) every
    rejection rule lies first, in the middle, last and at sectors 255, 256, 1023, 1024, 4095 and 4096 of some run, and
    a long run has a bad sector every few hundred"""
    rules = sc.rules_for(mlp)
    assert [p for p, r in sc.bad_plan(1, 0, rules)] == []
    assert [p for p, r in sc.bad_plan(3, 0, rules)] == [0]
    assert [p for p, r in sc.bad_plan(5, 0, rules)] == [0, 2, 4]
    seen = set()
    for index in range(len(rules) if mlp else len(sc.LAYOUTS)):
        for n in sc.COUNTS:
            plan = sc.bad_plan(n, sc.run_shift(index, n), rules)
            pos = [p for p, r in plan]
            assert len(set(pos)) == len(pos) and max(np.diff([-1] + pos + [n]), default=0) <= 520
            seen |= {(role, r) for p, r in plan for role in sc.roles(p, n)}
            if n == 5121:
                assert len(plan) >= 24 and {0, 255, 256, 1023, 1024, 2560, 4095, 4096, 5120} <= set(pos)
                assert set(rules) == {r for p, r in plan}            # every rule in every long run
    want = {(role, r) for role in ("first", "middle", "last") + sc.EDGES for r in rules}
    assert want <= seen, sorted(want - seen, key=str)


# ------------------------------------------------------------------------------------------------ model vs muxer
@pytest.mark.parametrize("bps,ch,asg", sc.LAYOUTS)
def test_model_recovers_the_muxed_samples(bps, ch, asg):
    lim = 1 << (bps - 1)
    secs, want = [], []
    for i, (name, sh) in enumerate(sc.SECTOR_SHAPES.items()):
        sec, s, _ = sc.pcm_sector(sh, bps, ch, asg, i)
        secs.append(sec)
        want.append(s)
    m = sc.model_pcm(np.frombuffer(b"".join(secs), np.uint8), bps, ch)
    assert m.bad == 0
    assert [int(c) for c in m.counts] == [len(s) for s in want]
    every = np.concatenate(want)
    assert (every == -lim).all(axis=1).any() and (every == lim - 1).all(axis=1).any()   # both rails, every channel
    block = sc.swizzle(sc.pattern_samples(bps, ch, 1, 5), bps)
    assert len(set(block)) == len(block) == 2 * ch * (bps // 8)      # every byte of a chunk differs from the others
    assert np.array_equal(m.pcm, np.concatenate(want).T)
    assert np.array_equal(m.base, np.concatenate([[0], np.cumsum([len(s) for s in want])]))


def test_model_recovers_the_muxed_mlp_bytes():
    data, sectors = _mlp_run()
    m = sc.model_mlp(sectors)
    assert m.bad == 0 and len(m.mlp) >= len(data)
    assert np.array_equal(m.mlp[:len(data)], data) and not m.mlp[len(data):].any()


def test_model_counts_a_bad_sector_and_takes_nothing_from_it():
    good = [sc.pcm_sector(sc.SECTOR_SHAPES[n], 24, 3, 2, i) for i, n in enumerate(("two", "off3", "eight"))]
    for rule in sc.RULES:
        data = np.frombuffer(good[0][0] + sc.malformed(rule, 24, 2) + sc.malformed(rule, 24, 2) + good[1][0] +
                             good[2][0], np.uint8)
        m = sc.model_pcm(data, 24, 3)
        assert m.bad == 2 and m.reasons == {1: rule, 2: rule}
        assert np.array_equal(m.pcm, np.concatenate([g[1] for g in good]).T)


# ------------------------------------------------------------------------------------------------ model vs reference
def _ref_payload(pkg, tmp, sectors, frames):
    ats = pkg.disc.write_disc(tmp, [{"sectors": sectors, "pcm_frames": frames, "rate_code": 0}])
    wavs = _run(REF_TOOL, ats, os.path.join(tmp, "out"))
    assert len(wavs) == 1
    return (np.frombuffer(open(wavs[0], "rb").read()[68:], np.uint8),)      # behind the 68-byte EXTENSIBLE header


@pytest.mark.parametrize("bps,ch,asg", REF_LAYOUTS)
def test_model_equals_reference_dvda2wav_pcm(pkg, bps, ch, asg):
    """every well-formed shape that tiles exactly, as a one-track disc through the reference's own tool: the pack
    stuffing, pad_1, pad_2, non-audio packets and several audio packets per sector are the reference's rules, not only
    this project's reading of them"""
    for name, sh in sc.SECTOR_SHAPES.items():
        if sh["stray"]:
            continue
        sec, s, _ = sc.pcm_sector(sh, bps, ch, asg, 2)
        m = sc.model_pcm(np.frombuffer(sec, np.uint8), bps, ch)
        assert m.bad == 0 and m.base[-1] == len(s)
        want = sc.wav_payload(m.pcm, bps)
        with tempfile.TemporaryDirectory() as tmp:
            assert oracle_lib.same_as_reference("sector_pcm_%d_%d_%s" % (bps, ch, name), (want,),
                                                lambda: _ref_payload(pkg, tmp, [sec], len(s))), name


def _au_lengths(data):
    out, pos = [], 0
    while pos + 4 <= len(data):
        n = 2 * (((int(data[pos]) << 8) | int(data[pos + 1])) & 0xFFF)
        out.append(n)
        pos += n
    return out


def test_model_equals_reference_dvda2wav_mlp(pkg, oracle):
    """the same sector shapes carrying a short MLP stream; the expected PCM is the oracle's decode of the stream.
    Shapes with a packet too short to complete an access unit are left to the model: the reference ends the track at
    such a packet (the third divergence above)."""
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=1, rate_code=0, n_substreams=1, n_aus=24)
    data, frames = syn.stream(cfg, 5)
    pcm, r, st = oracle.decode(data, 2, frames)
    assert st == 0 and r == frames
    want = sc.wav_payload(pcm, 24)
    longest = max(_au_lengths(data))
    ran = []
    for name, sh in sc.MLP_SHAPES.items():
        if sh["stray"]:
            continue
        secs = sc.mlp_sectors([name], data)
        m = sc.model_mlp(np.frombuffer(b"".join(secs), np.uint8))
        assert m.bad == 0 and np.array_equal(m.mlp[:len(data)], data)
        if min(ln for d, ln, off in m.packets if d + ln <= len(data)) < longest:
            continue
        ran.append(name)
        with tempfile.TemporaryDirectory() as tmp:
            assert oracle_lib.same_as_reference("sector_mlp_%s" % name, (want,),
                                                lambda: _ref_payload(pkg, tmp, secs, frames)), name
    # every payload offset & 3, one, two and three packets per sector, other packets between them, a payload to byte 2047
    assert {"c63", "c64", "c65", "most", "most_off2", "to_the_end", "mlp_no_pad2", "mlp_big2", "mlp_big3"} <= set(ran)


def test_reference_ends_a_track_where_the_kernels_go_on(pkg):
    """the three known divergences on two-sector tracks: what the reference's tool writes is the model's output cut at
    the place named"""
    bps, ch, asg = 16, 2, 1
    plain, s_plain, _ = sc.pcm_sector(sc.SECTOR_SHAPES["off1"], bps, ch, asg, 9)
    stray, s_stray, _ = sc.pcm_sector(sc.SECTOR_SHAPES["stray1"], bps, ch, asg, 1)
    hole = sc.shape([sc.A(("c", 3, 0)), sc.A(("c", 0, 1)), sc.A(("c", 5, 0))])
    holed, s_hole, _ = sc.pcm_sector(hole, bps, ch, asg, 2)
    other = plain.replace(sc.params_block(bps, asg), sc.params_block(bps, asg, 1))      # 96 kHz in a 48 kHz track
    assert other != plain
    cases = {"stray": ([stray, plain], len(s_stray)),             # nothing behind the sector with the stray byte
             "no_frame": ([holed, plain], 6),                     # nothing behind the packet without a whole chunk
             "params": ([plain, other], len(s_plain))}
    for key, (secs, kept) in cases.items():
        m = sc.model_pcm(np.frombuffer(b"".join(secs), np.uint8), bps, ch)
        assert m.bad == 0 and m.base[-1] > kept                   # the model, like the kernels, keeps all of it
        want = sc.wav_payload(m.pcm[:, :kept], bps)
        with tempfile.TemporaryDirectory() as tmp:
            assert oracle_lib.same_as_reference("sector_divergence_%s" % key, (want,),
                                                lambda: _ref_payload(pkg, tmp, secs, int(m.base[-1]))), key
