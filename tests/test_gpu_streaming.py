"""The streaming tier (csrc/mlp_stream.c, csrc/mlp_stepper.h, k_coop<false, true>) where its two copies of the decoder
state have to agree: the late hand-over from the stepping kernel to the batch-tier path, packets cut at and around every
unit boundary and down to single bytes, the 44.1 kHz family and the odd channel assignments, damage, several decoders
alive at once.  The cases are tests/streaming_cases.py's; tests/test_streaming_model.py holds their premises on the CPU.

Every case feeds hip.MLPDecoder and the oracle's decode_packet (= the reference's mlp.h) the same packets side by side
and keeps a record per call; a failure names the first differing call, channel and frame."""
import collections

import numpy as np
import pytest

from tests import streaming_cases as sc
from tests.stream_tools import cuts_at_units, frame_offsets

pytestmark = pytest.mark.gpu

Call = collections.namedtuple("Call", "size got want status path queued")
Run = collections.namedtuple("Run", "calls pcm want_pcm want_status")


def feed(hip, oracle, c, data, cuts, params=None, extra=()):
    """`data` cut at `cuts` (then the packets of `extra`) through hip.MLPDecoder and the oracle, side by side
    -> Run(one Call per packet, the PCM handed out [channels, frames], the oracle's PCM, the oracle's status)"""
    cfg = c.cfg
    dec = hip.MLPDecoder(*(params or (cfg.bps_code, cfg.bps_code, cfg.rate_code, cfg.rate_code, cfg.assignment)))
    od = sc.OracleDecoder(oracle, c.nch)
    samples = [[] for _ in range(6)]
    calls = []
    try:
        for piece in list(sc.packets(data, cuts)) + list(extra):
            want = od.decode_packet(piece)
            got = dec.decode_packet(piece, samples)
            calls.append(Call(len(piece), got, want, dec.status, dec.path, dec.queued_bytes))
        want_pcm, want_status = od.pcm(), od.status
    finally:
        od.close()
        dec.close()
    assert len({len(s) for s in samples[:c.nch]}) == 1 and not any(samples[c.nch:])
    pcm = np.asarray(samples[:c.nch], np.int32).reshape(c.nch, -1)
    assert pcm.shape[1] == sum(k.got for k in calls)
    return Run(calls, pcm, want_pcm, want_status)


def first_difference(run):
    """the first call whose return or whose PCM differs from the oracle's, with channel and frame"""
    lo = 0
    for i, k in enumerate(run.calls):
        if k.got != k.want:
            return "call %d (%d bytes): returned %d, the oracle %d" % (i, k.size, k.got, k.want)
        a, b = run.pcm[:, lo:lo + k.got], run.want_pcm[:, lo:lo + k.got]
        if not np.array_equal(a, b):
            ch, fr = np.argwhere(a != b)[0]
            return "call %d (%d bytes, frames %d..%d, path %d): channel %d frame %d is %d, the oracle %d" % (
                i, k.size, lo, lo + k.got, k.path, ch, lo + fr, a[ch, fr], b[ch, fr])
        lo += k.got
    return None


def assert_exact(hip, run, end_path=None):
    """every call's return is the oracle's, the PCM is bit-exact, the status stays benign"""
    bad = [i for i, k in enumerate(run.calls) if k.status & ~hip.ST_BENIGN]
    assert not bad, "call %d: status %#x" % (bad[0], run.calls[bad[0]].status)
    assert run.want_status == 0
    diff = first_difference(run)
    assert diff is None, diff
    assert run.pcm.shape == run.want_pcm.shape
    assert run.calls[-1].queued < 4
    if end_path is not None:
        assert run.calls[-1].path == end_path
    # an empty packet returns 0 and changes nothing
    for i, k in enumerate(run.calls):
        if k.size == 0 and i:
            assert k.got == 0 and (k.status, k.path, k.queued) == run.calls[i - 1][3:], "empty packet, call %d" % i


# ------------------------------------------------------------------------------------------ a. late hand-over
@pytest.mark.parametrize("pack", sorted(sc.PACKETISATIONS))
@pytest.mark.parametrize("name", sc.HANDOVER)
def test_late_hand_over(pkg, oracle, name, pack):
    """A stream the stepping kernel has decoded for many units -- queue cut at several syncs, a FIR history fetched from
    the device, frames of the kept segment handed out -- meets a unit it does not take (larger than its stage:
    DVDA_ST_SEQ; of non-standard length: DVDA_ST_TIMING) and goes on, from those three things, on the batch-tier path.
    path is 0 up to the call in front of the one that completes that unit and 1 from it on: the switch was late.
    (What each of the three catches: a `rows_before` off by a unit changes a call's return in every fixture whose trigger
    lies behind a queue cut; a lost `fir` changes PCM that is handed out only in streaming_cases.KEPT_HISTORY fed one
    unit per call -- elsewhere the wrong values have died out inside frames handed out before, see there.)"""
    hip = pkg.hipdec
    c = sc.case(pkg.synth, name)
    cuts = sc.PACKETISATIONS[pack](c.data)
    run = feed(hip, oracle, c, c.data, cuts)
    assert_exact(hip, run, end_path=1)
    if pack == "whole":
        return
    turn = sc.call_completing(cuts, sc.unit_bounds(c.data)[c.trigger + 1])
    assert turn >= 1
    paths = [k.path for k in run.calls]
    assert paths[:turn] == [0] * turn, "left the stepping kernel in call %d, the trigger unit is complete in call %d" % (
        paths.index(1), turn)
    assert paths[turn:] == [1] * (len(paths) - turn), "call %d completes the trigger unit: path %s" % (turn, paths[turn:])
    if c.trigger >= 4:
        assert sum(k.got for k in run.calls[:turn]) >= 2 * c.rpa        # the stepping kernel did decode in front of it


# ------------------------------------------------------------------------------------------ b. every boundary
@pytest.mark.parametrize("pack", ["units", "around"])
@pytest.mark.parametrize("name", sorted(sc.BOUNDARY))
def test_every_unit_boundary(pkg, oracle, name, pack):
    """One access unit per call: the whole device state (parameters, matrices, seeds, FIR and IIR histories, with IIR
    taps, six matrices, changes and restarts inside units, syncs that restart nothing) crosses a call at every boundary;
    and cuts one byte before and one byte after every boundary."""
    hip = pkg.hipdec
    c = sc.case(pkg.synth, name)
    cuts = cuts_at_units(c.data) if pack == "units" else sc.cuts_around_units(c.data)
    run = feed(hip, oracle, c, c.data, cuts)
    assert_exact(hip, run, end_path=0)
    if pack == "units":
        assert [k.got for k in run.calls] == [c.rpa] * len(cuts)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("name", sorted(sc.SMALL))
def test_packets_shorter_than_a_unit_header(pkg, oracle, name, n):
    hip = pkg.hipdec
    c = sc.case(pkg.synth, name)
    cuts = sc.cuts_tiny(c.data, n)
    run = feed(hip, oracle, c, c.data, cuts)
    assert_exact(hip, run, end_path=0)
    assert sum(1 for k in run.calls if k.size == 0) >= 10 and sum(1 for k in run.calls if k.got) == 12


# ------------------------------------------------------------------------------------------ c. other layouts
@pytest.mark.parametrize("pack", ["p2011", "units"])
@pytest.mark.parametrize("name", sorted(sc.LAYOUTS))
def test_other_rates_and_assignments(pkg, oracle, name, pack):
    """rows_per_au() exists three times (mlp_stream.c, the stepper, the kernel): the 44.1 kHz family and the 1-, 3-, 5-
    and 6-channel (0x14) assignments through decode_packet"""
    hip = pkg.hipdec
    c = sc.case(pkg.synth, name)
    run = feed(hip, oracle, c, c.data, sc.PACKETISATIONS[pack](c.data))
    assert_exact(hip, run, end_path=0)
    assert run.pcm.shape == (c.nch, c.frames)


# ------------------------------------------------------------------------------------------ d. damage
_clean = {}


def clean_pcm(pkg, oracle, name):
    if name not in _clean:
        c = sc.case(pkg.synth, name)
        pcm, r, st = oracle.decode(c.data, c.nch, c.frames)
        assert st == 0 and r == c.frames
        pcm.setflags(write=False)
        _clean[name] = pcm
    return _clean[name]


def assert_stopped(hip, run, clean, first_bad):
    """from call `first_bad` on: a non-benign status that no later call changes, every later call returns 0 and queues
    nothing; what was handed out is a prefix of the clean stream's PCM"""
    calls = run.calls
    bad = [i for i, k in enumerate(calls) if k.status & ~hip.ST_BENIGN]
    assert bad and bad[0] == first_bad, "stopped in call %s, expected in call %d" % (bad[:1], first_bad)
    for i in range(first_bad + 1, len(calls)):
        assert calls[i].got == 0 and (calls[i].status, calls[i].queued) == (calls[first_bad].status, calls[first_bad].queued), \
            "call %d after the stop: returned %d, status %#x, %d queued" % (i, calls[i].got, calls[i].status, calls[i].queued)
    total = run.pcm.shape[1]
    assert total <= clean.shape[1]
    if not np.array_equal(run.pcm, clean[:, :total]):
        ch, fr = np.argwhere(run.pcm != clean[:, :total])[0]
        pytest.fail("handed out %d frames, not a prefix of the clean PCM: channel %d frame %d" % (total, ch, fr))
    return total


@pytest.mark.parametrize("pack", sorted(sc.PACKETISATIONS))
@pytest.mark.parametrize("kind,k", [(kind, k) for kind in sc.DAMAGE_KINDS for k in sc.DAMAGE_UNITS] + [("nosync", 0)])
@pytest.mark.parametrize("base", sc.DAMAGE_BASES)
def test_damage_stops_the_decoder(pkg, oracle, base, kind, k, pack):
    """Where the reference assert()s or stalls, the tier hands out what the steps in front of the failing one decoded --
    a prefix of the clean PCM, of exactly the length mlp_stream.c's `failed` branch fixes --, says why, and stays
    stopped: later calls return 0 and queue nothing.  A decoder opened afterwards is not affected."""
    hip = pkg.hipdec
    c = sc.case(pkg.synth, base)
    clean = clean_pcm(pkg, oracle, base)
    d, ku = sc.damaged(c.data, kind, k)
    # (the cuts are the clean stream's: a size field below 4 ends the unit chain; without the first unit, its own)
    cuts = sc.PACKETISATIONS[pack](d if kind == "nosync" else c.data)
    bounds = sc.unit_bounds(d if kind == "nosync" else c.data)
    later = [np.zeros(0, np.uint8), np.ascontiguousarray(c.data[:sc.PACKET])]
    run = feed(hip, oracle, c, d, cuts, extra=later)
    status = run.calls[-1].status
    if kind in ("flip", "crc"):
        units_out, units_before = sc.handed_out_before_failure(bounds, cuts, ku)
        total = assert_stopped(hip, run, clean, sc.call_completing(cuts, bounds[ku + 1]))
        assert units_before * c.rpa <= total <= ku * c.rpa
        assert total == units_out * c.rpa
        assert status & run.want_status & ~hip.ST_BENIGN & (hip.ST["PARITY"] | hip.ST["CRC"]), \
            "status %#x, the oracle's %#x" % (status, run.want_status)
    elif kind == "size":
        # the units in front of the header are decoded as the oracle decodes them, call by call
        total = assert_stopped(hip, run, clean, sc.call_completing(cuts, bounds[ku] + 4))
        assert status & hip.ST["EOF"] and run.want_status & hip.ST["EOF"]
        assert total == ku * c.rpa == run.want_pcm.shape[1]
        assert [x.got for x in run.calls[:len(cuts)]] == [x.want for x in run.calls[:len(cuts)]]
    else:
        total = assert_stopped(hip, run, clean, sc.call_completing(cuts, bounds[1]))
        assert status & hip.ST["NO_SYNC"] and run.want_status & hip.ST["NO_SYNC"] and total == 0
    after = feed(hip, oracle, c, c.data, sc.cuts_whole(c.data))
    assert_exact(hip, after, end_path=0)
    assert np.array_equal(after.pcm, clean)


# ------------------------------------------------------------------------------------------ e. several decoders
def test_several_decoders_alive_at_once(pkg, oracle):
    """Each decoder has its own device state, pinned buffers and stream: three fed alternately, one packet each in
    turn, a fourth between them that stops at a flipped bit; then all closed and one more opened and run."""
    syn, hip = pkg.synth, pkg.hipdec
    names = ["s1r1", "s2r1_pad21", "small_2ch_48k", "recipe_2ss_40"]
    cs = [sc.case(syn, n) for n in names]
    datas = [c.data for c in cs[:3]] + [sc.damaged(cs[3].data, "flip", 17)[0]]
    chunk = [777, 777, 199, 777]
    cutss = [sc.cuts_fixed(d, n) for d, n in zip(datas, chunk)]
    decs = [hip.MLPDecoder(c.cfg.bps_code, c.cfg.bps_code, c.cfg.rate_code, c.cfg.rate_code, c.cfg.assignment) for c in cs]
    samples = [[[] for _ in range(6)] for _ in cs]
    rets = [[] for _ in cs]
    stat = [[] for _ in cs]
    try:
        feeds = [list(sc.packets(d, cuts)) for d, cuts in zip(datas, cutss)]
        for i in range(max(len(f) for f in feeds)):
            for j in (0, 3, 1, 2):
                if i < len(feeds[j]):
                    rets[j].append(decs[j].decode_packet(feeds[j][i], samples[j]))
                    stat[j].append((decs[j].status, decs[j].queued_bytes, decs[j].path))
        paths = [d.path for d in decs]
    finally:
        for d in decs:
            d.close()
    for j in range(3):
        want_rets, want, st = sc.oracle_calls(oracle, cs[j].nch, datas[j], cutss[j])
        assert st == 0 and all(s[0] & ~hip.ST_BENIGN == 0 for s in stat[j]), names[j]
        assert rets[j] == want_rets, names[j]
        got = np.asarray(samples[j][:cs[j].nch], np.int32)
        assert got.shape == want.shape and np.array_equal(got, want), names[j]
    assert paths[:3] == [0, 1, 0]
    # the fourth: stopped in the call that completes unit 17, a prefix handed out, nothing after
    b = sc.unit_bounds(cs[3].data)
    turn = sc.call_completing(cutss[3], b[18])
    units_out, _ = sc.handed_out_before_failure(b, cutss[3], 17)
    assert [bool(s[0] & ~hip.ST_BENIGN) for s in stat[3]] == [False] * turn + [True] * (len(stat[3]) - turn)
    assert sum(rets[3][:turn]) == units_out * 80 and not any(rets[3][turn:]) and len(set(stat[3][turn:])) == 1
    got = np.asarray(samples[3], np.int32)
    assert np.array_equal(got, clean_pcm(pkg, oracle, "recipe_2ss_40")[:, :units_out * 80])
    # all closed: one more
    c = sc.case(syn, "s2r1")
    assert_exact(hip, feed(hip, oracle, c, c.data, sc.cuts_fixed(c.data, sc.PACKET)), end_path=0)


# ------------------------------------------------------------------------------------------ f. open parameters
@pytest.mark.parametrize("name", ["s2r1", "small_mono_44k", "s1r1_pad18"])
def test_open_parameters_are_ignored(pkg, oracle, name):
    """As in the reference (src/mlp.c:273 stores the parameters; nothing reads them): a decoder opened with
    parameters that contradict the stream decodes by the stream's major sync."""
    hip = pkg.hipdec
    c = sc.case(pkg.synth, name)
    cuts = sc.cuts_fixed(c.data, sc.PACKET)
    wrong = (0, 1, 10 if c.cfg.rate_code != 10 else 0, 8, 1 if c.nch != 2 else 12)
    run = feed(hip, oracle, c, c.data, cuts, params=wrong)
    assert_exact(hip, run, end_path=1 if c.trigger is not None else 0)
    assert run.pcm.shape == (c.nch, len(frame_offsets(c.data)) * c.rpa)
