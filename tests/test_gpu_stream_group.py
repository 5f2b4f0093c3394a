"""A group of streaming-tier decoders stepped by one launch pair (csrc/mlp_stream.c decode_many, csrc/mlp_stepper.h,
k_coop<false, true> with a workgroup per member): every member behaves as a lone decoder fed the same packets.

The fixtures and packetisations are tests/streaming_cases.py's.  Every member is fed next to the oracle's decode_packet
(= the reference's mlp.h) and, where a test says so, next to a lone hip.MLPDecoder; a record is kept per member and call,
and a failure names member, call, channel and frame."""
import collections

import numpy as np
import pytest

from tests import streaming_cases as sc
from tests.stream_tools import cuts_at_units

pytestmark = pytest.mark.gpu

Call = collections.namedtuple("Call", "size got want status path queued lone")
Run = collections.namedtuple("Run", "name calls pcm want_pcm want_status")
Member = collections.namedtuple("Member", "name case data pieces")

PACKS = {"p2011": lambda d: sc.cuts_fixed(d, sc.PACKET), "units": cuts_at_units, "around": sc.cuts_around_units,
         "tiny3": lambda d: sc.cuts_tiny(d, 3), "whole": sc.cuts_whole}
MIXED = [("s1r1", "p2011"), ("s2r2", "units"), ("rich_s1", "around"), ("rich_s2_synconly", "whole"), ("rate9", "units"),
         ("asg0", "around"), ("asg0x14", "p2011"), ("small_mono_44k", "tiny3")]


def member(pkg, name, pack, data=None, delay=0):
    """fixture `name` (or `data`, a damaged copy of it) cut by `pack`, fed from call `delay` on"""
    c = sc.case(pkg.synth, name)
    data = c.data if data is None else data
    return Member(name, c, data, [None] * delay + list(sc.packets(data, PACKS[pack](data))))


def feed_group(hip, oracle, members, lone=False, tail=0):
    """One hip.MLPDecoderGroup call per row of the members' packets (a member that has run out gets None), `tail` more
    calls with nothing for anybody; beside it the oracle and, lone=True, a hip.MLPDecoder per member, fed the same packets
    -> ([Run per member], [group.steps after every call])"""
    n = len(members)
    n_calls = max(len(m.pieces) for m in members) + tail
    group = hip.MLPDecoderGroup(n)
    ods = [sc.OracleDecoder(oracle, m.case.nch) for m in members]
    lones = []
    samples = [[[] for _ in range(6)] for _ in range(n)]
    lone_samples = [[[] for _ in range(6)] for _ in range(n)]
    calls = [[] for _ in range(n)]
    steps = []
    try:
        if lone:
            for m in members:
                cfg = m.case.cfg
                lones.append(hip.MLPDecoder(cfg.bps_code, cfg.bps_code, cfg.rate_code, cfg.rate_code, cfg.assignment))
        for k in range(n_calls):
            pieces = [m.pieces[k] if k < len(m.pieces) else None for m in members]
            want = [ods[i].decode_packet(p) if p is not None else 0 for i, p in enumerate(pieces)]
            got = group.decode_packets(pieces, samples)
            steps.append(group.steps)
            for i, p in enumerate(pieces):
                rec = None
                if lone:
                    d = lones[i]
                    r = d.decode_packet(p, lone_samples[i]) if p is not None else 0
                    rec = (r, d.status, d.path, d.queued_bytes)
                calls[i].append(Call(0 if p is None else len(p), got[i], want[i], group.status(i), group.path(i),
                                     group.queued_bytes(i), rec))
        runs = []
        for i, m in enumerate(members):
            nch = m.case.nch
            assert len({len(s) for s in samples[i][:nch]}) == 1 and not any(samples[i][nch:]), "member %d (%s)" % (i, m.name)
            pcm = np.asarray(samples[i][:nch], np.int32).reshape(nch, -1)
            assert pcm.shape[1] == sum(c.got for c in calls[i]), "member %d (%s)" % (i, m.name)
            if lone:
                assert samples[i] == lone_samples[i], "member %d (%s): PCM differs from the lone decoder's" % (i, m.name)
            runs.append(Run(m.name, calls[i], pcm, ods[i].pcm(), ods[i].status))
        return runs, steps
    finally:
        for od in ods:
            od.close()
        for d in lones:
            d.close()
        group.close()


def first_difference(i, run):
    """the first call of member i whose return or whose PCM differs from the oracle's, with channel and frame"""
    lo = 0
    who = "member %d (%s), " % (i, run.name)
    for j, k in enumerate(run.calls):
        if k.got != k.want:
            return who + "call %d (%d bytes): returned %d, the oracle %d" % (j, k.size, k.got, k.want)
        a, b = run.pcm[:, lo:lo + k.got], run.want_pcm[:, lo:lo + k.got]
        if not np.array_equal(a, b):
            ch, fr = np.argwhere(a != b)[0]
            return who + "call %d (%d bytes, frames %d..%d, path %d): channel %d frame %d is %d, the oracle %d" % (
                j, k.size, lo, lo + k.got, k.path, ch, lo + fr, a[ch, fr], b[ch, fr])
        lo += k.got
    return None


def assert_exact(hip, i, run, end_path=None):
    """every call's return is the oracle's, the PCM is bit-exact, the status stays benign, nothing is left queued"""
    who = "member %d (%s)" % (i, run.name)
    bad = [j for j, k in enumerate(run.calls) if k.status & ~hip.ST_BENIGN]
    assert not bad, "%s, call %d: status %#x" % (who, bad[0], run.calls[bad[0]].status)
    assert run.want_status == 0, who
    diff = first_difference(i, run)
    assert diff is None, diff
    assert run.pcm.shape == run.want_pcm.shape, who
    assert run.calls[-1].queued < 4, who
    if end_path is not None:
        assert run.calls[-1].path == end_path, who
    for j, k in enumerate(run.calls):       # a call without a packet returns 0 and changes nothing
        if k.size == 0 and j:
            assert k.got == 0 and (k.status, k.path, k.queued) == run.calls[j - 1][3:6], "%s: empty packet, call %d" % (who, j)


def assert_as_lone(i, run):
    """call for call: the lone decoder's return, status, path and queued bytes"""
    for j, k in enumerate(run.calls):
        assert (k.got, k.status, k.path, k.queued) == k.lone, (
            "member %d (%s), call %d (%d bytes): (return, status, path, queued) is %r, the lone decoder's %r" % (
                i, run.name, j, k.size, (k.got, k.status, k.path, k.queued), k.lone))


# ------------------------------------------------------------------------------------------ 1, 2: a mixed group
@pytest.fixture(scope="module")
def mixed(pkg, oracle):
    members = [member(pkg, name, pack) for name, pack in MIXED]
    return members, feed_group(pkg.hipdec, oracle, members, lone=True)[0]


def test_mixed_group_mixed_packetisations(pkg, mixed):
    """Substream counts, rates, channel counts and the IIR / six-matrix / mid-unit-restart state all differ between
    neighbouring workgroups, and so does what a call brings: a state record or a result slot indexed by the wrong member
    shows here."""
    members, runs = mixed
    for i, run in enumerate(runs):
        assert_exact(pkg.hipdec, i, run, end_path=0)
    # (by the oracle's returns) one and the same call completes no unit for one member that was fed bytes, one unit for
    # another and several for a third; and a member gets an empty packet in a call that decodes for others
    kinds = [{(0 if k.want == 0 else 1 if k.want == m.case.rpa else 2) for m, r in zip(members, runs)
              for k in [r.calls[j]] if k.size} for j in range(len(runs[0].calls))]
    assert any(s == {0, 1, 2} for s in kinds)
    assert any(p is not None and len(p) == 0 and any(r.calls[j].want for r in runs)
               for m in members for j, p in enumerate(m.pieces))


def test_group_equals_lone_decoders(mixed):
    for i, run in enumerate(mixed[1]):
        assert_as_lone(i, run)


# ------------------------------------------------------------------------------------------ 3: what a caller pays
def test_one_launch_pair_per_call(pkg, oracle):
    members = [member(pkg, name, "units") for name, _ in MIXED]
    # (behind the data: a call with an empty packet for everybody, then calls with none)
    longest = max(len(m.pieces) for m in members)
    members = [m._replace(pieces=m.pieces + [None] * (longest - len(m.pieces)) + [np.zeros(0, np.uint8)]) for m in members]
    runs, steps = feed_group(pkg.hipdec, oracle, members, tail=3)
    for i, run in enumerate(runs):
        assert_exact(pkg.hipdec, i, run, end_path=0)
    assert steps[:longest] == list(range(1, longest + 1))
    assert steps[longest:] == [longest] * 4


# ------------------------------------------------------------------------------------------ 4: rounds
def test_rounds_within_one_call(pkg, oracle):
    """a member that brings more than one step takes makes the call several rounds; the others take part in the first"""
    members = [member(pkg, "r2_6ch_60", "whole"), member(pkg, "s1r1", "p2011"), member(pkg, "small_2ch_48k", "units")]
    runs, steps = feed_group(pkg.hipdec, oracle, members)
    for i, run in enumerate(runs):
        assert_exact(pkg.hipdec, i, run, end_path=0)
    bounds = sc.unit_bounds(members[0].data)
    want = sc.steps_of_call(bounds, 0, len(bounds) - 1)
    assert len(want) > 1
    assert steps[0] == len(want)
    assert steps[1] == steps[0] + 1


# ------------------------------------------------------------------------------------------ 5: hand-over
def test_a_member_hands_over_while_the_others_go_on(pkg, oracle):
    spec = [("s2r1_pad18", "p2011"), ("splice_s1r1", "units"), ("fir_s2r0_pad33", "units"), ("s1r1", "p2011"),
            ("rich_s2", "units")]
    members = [member(pkg, name, pack) for name, pack in spec]
    runs, _ = feed_group(pkg.hipdec, oracle, members)
    for i, (m, run) in enumerate(zip(members, runs)):
        assert_exact(pkg.hipdec, i, run, end_path=1 if i < 3 else 0)
        paths = [k.path for k in run.calls]
        if i >= 3:
            assert paths == [0] * len(paths), "member %d (%s) left the stepping path" % (i, m.name)
            continue
        cuts = PACKS[spec[i][1]](m.data)
        turn = sc.call_completing(cuts, sc.unit_bounds(m.data)[m.case.trigger + 1])
        assert turn >= 1
        assert paths[:turn] == [0] * turn, "member %d (%s) left the stepping path in call %d, its trigger unit is complete in call %d" % (
            i, m.name, paths.index(1), turn)
        assert paths[turn:] == [1] * (len(paths) - turn), "member %d (%s): call %d completes the trigger unit, paths %s" % (
            i, m.name, turn, paths[turn:])


# ------------------------------------------------------------------------------------------ 6: damage
def test_damage_stays_with_its_member(pkg, oracle):
    hip = pkg.hipdec
    d0, _ = sc.damaged(sc.case(pkg.synth, "recipe_2ss_40").data, "crc", 17)
    d1, _ = sc.damaged(sc.case(pkg.synth, "r2_6ch_60").data, "size", 1)
    members = [member(pkg, "recipe_2ss_40", "p2011", data=d0), member(pkg, "r2_6ch_60", "p2011", data=d1),
               member(pkg, "s1r1", "p2011"), member(pkg, "rich_s1", "units")]
    runs, _ = feed_group(hip, oracle, members, lone=True)
    for i in (0, 1):
        run = runs[i]
        assert_as_lone(i, run)
        stopped = [j for j, k in enumerate(run.calls) if k.status & ~hip.ST_BENIGN]
        assert stopped, "member %d (%s) never stopped" % (i, run.name)
        first = stopped[0]
        assert first < len(members[i].pieces) - 1       # (packets were still to come)
        for j in range(first + 1, len(run.calls)):
            k = run.calls[j]
            assert k.got == 0 and k.queued == run.calls[first].queued and k.status == run.calls[first].status, (
                "member %d (%s), call %d behind the stop in call %d: %r" % (i, run.name, j, first, k))
    for i in (2, 3):
        assert_exact(hip, i, runs[i], end_path=0)


# ------------------------------------------------------------------------------------------ 7: many members
@pytest.mark.parametrize("n", [1, 5, 70])
def test_more_members_than_a_wave_has_lanes(pkg, oracle, n):
    """70: more members than a wave has lanes and than the decode summary has parts"""
    names = ["small_2ch_48k", "small_mono_44k", "asg2"]
    members = [member(pkg, names[i % 3], "units") for i in range(n)]
    runs, steps = feed_group(pkg.hipdec, oracle, members)
    for i, run in enumerate(runs):
        assert_exact(pkg.hipdec, i, run, end_path=0)
    assert steps[-1] == max(len(m.pieces) for m in members)


# ------------------------------------------------------------------------------------------ 8: slots over time
def test_slots_are_not_mixed_up_over_time(pkg, oracle):
    """a member that starts ten calls late (its `fresh` is its own, not the call's) and one that finishes early"""
    members = [member(pkg, "small_2ch_48k", "units"), member(pkg, "s1r1", "p2011"),
               member(pkg, "rich_s2", "whole", delay=10), member(pkg, "s2r2", "units")]
    assert 10 < len(members[0].pieces) < len(members[1].pieces) < len(members[3].pieces)
    runs, _ = feed_group(pkg.hipdec, oracle, members)
    for i, run in enumerate(runs):
        assert_exact(pkg.hipdec, i, run, end_path=0)
    assert [k.got for k in runs[2].calls[:10]] == [0] * 10 and runs[2].calls[10].got == runs[2].pcm.shape[1] > 0


# ------------------------------------------------------------------------------------------ 9: bounds
def test_bounds(pkg):
    hip = pkg.hipdec
    assert hip.STREAM_GROUP_MAX == 256
    for n in (0, hip.STREAM_GROUP_MAX + 1):
        with pytest.raises(hip.HipError):
            hip.MLPDecoderGroup(n)
    g = hip.MLPDecoderGroup(3)
    try:
        assert hip.lib().dvda_hip_mlpdecoder_group_size(g._h) == 3
        for i in (3, 4, 2 ** 31):
            assert g.status(i) == 0xFFFFFFFF and g.path(i) == -1 and g.queued_bytes(i) == 0
        assert (g.status(2), g.path(2), g.queued_bytes(2), g.steps) == (0, 0, 0, 0)
    finally:
        g.close()
