"""Streaming tier, CPU side: the premises of tests/test_gpu_streaming.py, held on the oracle, so that the GPU file cannot
pass for a reason other than the one it is written for -- every fixture of tests/streaming_cases.py decodes clean, the
restatement equals the compiled reference on it, the unit that triggers the fall-back is where the table says (late, behind
several queue cuts), the FIR history the tier carries over the hand-over changes the PCM, and each damage is one the
oracle reports at the unit it was put in."""
import numpy as np
import pytest

from tests import oracle_lib
from tests import streaming_cases as sc
from tests.stream_tools import cuts_at_units, frame_offsets, is_major_sync, major_syncs, splice

ORA_PARITY, ORA_CRC, ORA_EOF, ORA_NO_SYNC = 1 << 2, 1 << 3, 1 << 4, 1 << 0

CLEAN = sorted(sc.BASES) + sc.HANDOVER + sorted(sc.BOUNDARY) + sorted(sc.SMALL) + sorted(sc.LAYOUTS) + list(sc.DAMAGE_BASES)

_whole = {}


def whole(pkg, oracle, name):
    """(pcm, frames, status, every unit's frames) of fixture `name`, decoded once"""
    if name not in _whole:
        c = sc.case(pkg.synth, name)
        pcm, r, st = oracle.decode(c.data, c.nch, len(frame_offsets(c.data)) * 2 * c.rpa)
        per_unit, pcm_u, st_u = sc.oracle_calls(oracle, c.nch, c.data, cuts_at_units(c.data))
        assert st_u == st and np.array_equal(pcm_u, pcm)        # (the oracle itself does not care where packets end)
        pcm.setflags(write=False)
        _whole[name] = (pcm, r, st, per_unit)
    return _whole[name]


def expected_frames(pkg, oracle, name):
    c = sc.case(pkg.synth, name)
    if c.frames is not None:
        return c.frames
    # a splice: the standard units in front of the tail, then what the generator says the tail's stream holds less
    # what its own units in front of the splice point hold
    var = sc.case(pkg.synth, name + "_var")
    head = var.data[:major_syncs(var.data)[sc.SPLICE_SYNC]]
    _, r_head, st = oracle.decode(head, var.nch, len(frame_offsets(head)) * 2 * var.rpa)
    assert st == 0
    return c.trigger * c.rpa + var.frames - r_head


@pytest.mark.parametrize("name", CLEAN)
def test_fixture_decodes_clean(pkg, oracle, name):
    c = sc.case(pkg.synth, name)
    pcm, r, st, per_unit = whole(pkg, oracle, name)
    assert st == 0
    assert r == expected_frames(pkg, oracle, name) == sum(per_unit) and pcm.shape == (c.nch, r)
    n_units = 60 if name == "r2_6ch_60" else 40 if name == "recipe_2ss_40" else 12 if name in sc.SMALL else 36
    assert len(frame_offsets(c.data)) == n_units <= 60
    assert sc.unit_bounds(c.data)[-1] == len(c.data)
    assert pcm.any(axis=1).all()                                # no channel is silence


@pytest.mark.parametrize("name", CLEAN)
def test_restatement_equals_the_compiled_reference(pkg, oracle, name):
    c = sc.case(pkg.synth, name)
    pcm, r, st, _ = whole(pkg, oracle, name)
    assert st == 0
    assert oracle_lib.same_as_reference(
        "streaming_%s" % name, (pcm, r),
        lambda: oracle_lib.Reference().decode(c.data, c.cfg.assignment, c.cfg.rate_code, c.cfg.bps_code, r))


@pytest.mark.parametrize("name", sc.HANDOVER)
def test_trigger_unit_is_where_the_table_says(pkg, oracle, name):
    """Everything in front of the trigger is what the stepping kernel takes (standard length, within its stage); the
    trigger is not.  Two or more restarting major syncs lie at or in front of it -- the queue has been cut, a FIR
    history has come down from the device -- except where the table means to fall back before any cut (unit 1)."""
    c = sc.case(pkg.synth, name)
    _, _, _, per_unit = whole(pkg, oracle, name)
    b = sc.unit_bounds(c.data)
    sizes = [b[i + 1] - b[i] for i in range(len(b) - 1)]
    nonstd = [i for i, n in enumerate(per_unit) if n != c.rpa]
    big = [i for i, n in enumerate(sizes) if n > 4096]
    if name in sc.SPLICES:
        assert big == [] and nonstd[0] == c.trigger == 20 and len(nonstd) > 1
    else:
        assert nonstd == [] and big == [c.trigger] and sizes[c.trigger] == sc.PAD_SIZE
    cuts_in_front = [u for u in sc.restarting_syncs(c.data, c.S) if u <= c.trigger]
    assert cuts_in_front[0] == 0
    if c.trigger == 1:
        assert cuts_in_front == [0]
    else:
        assert len(cuts_in_front) >= 2
    assert c.nch == 6
    # the padding changes no PCM
    m = name.rsplit("_pad", 1)
    if len(m) == 2:
        assert np.array_equal(whole(pkg, oracle, name)[0], whole(pkg, oracle, m[0])[0])


@pytest.mark.parametrize("name", [n for n in sc.HANDOVER if not n.endswith("_pad1")])
def test_history_in_front_of_the_hand_over_matters(pkg, oracle, name):
    """The bytes from a restarting major sync on, decoded alone -- that is: with a FIR history of zeros --, must not give
    the PCM of the whole decode, or a lost `fir` would pass.  Held for the sync the queue begins at when the fall-back
    decodes (the last one strictly in front of the trigger, unless that is unit 0, where there is no history) and for
    the last one at or in front of the trigger (the first cut the batch-tier path makes itself)."""
    c = sc.case(pkg.synth, name)
    pcm, r, _, per_unit = whole(pkg, oracle, name)
    offs = frame_offsets(c.data)
    rs = sc.restarting_syncs(c.data, c.S)
    chosen = {max(u for u in rs if u <= c.trigger)}
    if max(u for u in rs if u < c.trigger) > 0:
        chosen.add(max(u for u in rs if u < c.trigger))
    assert chosen and 0 not in chosen
    for u in sorted(chosen):
        first = sum(per_unit[:u])
        alone, r_alone, _ = oracle.decode(c.data[offs[u]:], c.nch, r)
        assert r_alone == r - first
        differs = np.argwhere(alone != pcm[:, first:])
        assert len(differs), "sync at unit %d: zero history gives the same PCM" % u
        # ... and from the segment's first frames on, not somewhere later by accident
        assert differs[:, 1].min() < c.rpa


@pytest.mark.parametrize("name", sc.KEPT_HISTORY)
def test_kept_history_reaches_the_pcm_a_fall_back_hands_out(pkg, oracle, name):
    """The test above is the weak form: in most fixtures the wrong values have left the PCM within the sync's own access
    unit (a predictor's memory is some tens of frames), and that unit was handed out by the call that cut the queue at
    it -- a fall-back that had lost `fir` would hand out the right frames all the same.  In these two the trigger is the
    unit right behind a restarting sync, and a zero history in front of that sync still changes the trigger unit's own
    frames: fed one unit per call, the fall-back's first frames are wrong without the kept history."""
    c = sc.case(pkg.synth, name)
    pcm, r, _, per_unit = whole(pkg, oracle, name)
    u = c.trigger - 1
    assert u in sc.restarting_syncs(c.data, c.S) and u >= 8
    first = sum(per_unit[:u])
    alone, _, _ = oracle.decode(c.data[frame_offsets(c.data)[u]:], c.nch, r)
    differs = np.argwhere(alone != pcm[:, first:])
    in_trigger = differs[(differs[:, 1] >= c.rpa) & (differs[:, 1] < 2 * c.rpa)]
    assert len(in_trigger) >= 40, "%d samples of the trigger unit differ" % len(in_trigger)


def test_calls_of_more_than_one_step(pkg, oracle):
    """What puts a fall-back or a failure into a later step of a call: the rate-2 streams are two steps in one call (24
    units fill 48 KB), the trigger 35 in the second; the 60-unit stream is three, unit 17 in the first and the last in the
    third."""
    syn = pkg.synth
    for w, want in ((1, 0), (4, 0), (18, 0), (21, 0), (35, 1)):
        c = sc.case(syn, "s2r2_pad%d" % w)
        steps = sc.steps_of_call(sc.unit_bounds(c.data), 0, 36)
        assert len(steps) == 2 and len(c.data) > sc.step_limits()[1]
        assert [i for i, (a, e) in enumerate(steps) if a <= w < e] == [want]
    c = sc.case(syn, "r2_6ch_60")
    steps = sc.steps_of_call(sc.unit_bounds(c.data), 0, 60)
    assert len(steps) == 3 and steps[0][0] <= 17 < steps[0][1] and steps[2][0] <= 59 < steps[2][1]
    assert 60 > sc.step_limits()[0]
    for name in ("s1r1", "s2r1", "recipe_2ss_40"):
        c = sc.case(syn, name)
        assert len(sc.steps_of_call(sc.unit_bounds(c.data), 0, len(frame_offsets(c.data)))) == 1


@pytest.mark.parametrize("base", sc.DAMAGE_BASES)
def test_each_damage_is_reported_at_its_unit(pkg, oracle, base):
    c = sc.case(pkg.synth, base)
    clean = whole(pkg, oracle, base)[0]
    b = sc.unit_bounds(c.data)
    cap = clean.shape[1]
    for kind, bit in (("flip", ORA_PARITY | ORA_CRC), ("crc", ORA_CRC), ("size", ORA_EOF)):
        for k in sc.DAMAGE_UNITS:
            d, ku = sc.damaged(c.data, kind, k)
            assert len(d) == len(c.data) and ku == k % (len(b) - 1)
            assert np.flatnonzero(d != c.data).min() >= b[ku] and np.flatnonzero(d != c.data).max() < b[ku + 1]
            # rejected with unit k in, clean without it
            _, r_in, st_in = oracle.decode(d[:b[ku + 1]], c.nch, cap)
            pcm_out, r_out, st_out = oracle.decode(d[:b[ku]], c.nch, cap)
            assert st_in & bit and st_in & ~0x200 & ~(ORA_PARITY | ORA_CRC | ORA_EOF) == 0, (kind, k, hex(st_in))
            assert st_out == 0 and r_in == r_out == ku * c.rpa
            assert np.array_equal(pcm_out, clean[:, :r_out])
            if kind == "flip":
                assert not is_major_sync(d, (b[ku] + b[ku + 1]) // 2 - 4) and (b[ku] + b[ku + 1]) // 2 >= b[ku] + 64
    d, _ = sc.damaged(c.data, "nosync", 0)
    assert len(d) == len(c.data) - b[1] and not is_major_sync(d, 0)
    assert oracle.decode(d, c.nch, cap)[2] & ORA_NO_SYNC


def test_packetisations(pkg):
    syn = pkg.synth
    for name in sorted(sc.BOUNDARY):
        c = sc.case(syn, name)
        inner = frame_offsets(c.data)[1:]
        assert cuts_at_units(c.data) == inner + [len(c.data)]
        around = sc.cuts_around_units(c.data)
        assert len(around) == 2 * len(inner) + 1 and around == sorted(around)
        assert all(o - 1 in around and o + 1 in around and o not in around for o in inner)
    # SYNCONLY: major syncs that restart nothing are there, and the queue is not cut at them
    for name in ("rich_s1_synconly", "rich_s2_synconly"):
        c = sc.case(syn, name)
        assert len(major_syncs(c.data)) > len(sc.restarting_syncs(c.data, c.S)) >= 2
    # packets below the 4-byte unit header, an empty one after every tenth: at most some 2 800 calls
    for name in sorted(sc.SMALL):
        c = sc.case(syn, name)
        assert len(c.data) <= 2800
        for n in (1, 2, 3, 5):
            cuts = sc.cuts_tiny(c.data, n)
            sizes = np.diff([0] + cuts)
            assert sizes.max() == n < 4 + 2 and cuts[-1] == len(c.data) and len(cuts) <= 2800
            assert (sizes == 0).sum() == (len(sc.cuts_fixed(c.data, n))) // 10
    assert sc.case(syn, "small_mono_44k").cfg.rate_code == 8 and sc.case(syn, "small_mono_44k").nch == 1
    assert {sc.case(syn, n).cfg.rate_code for n in sc.LAYOUTS} >= {8, 9, 10}
    assert {sc.case(syn, n).nch for n in sc.LAYOUTS} == {1, 3, 5, 6}
    a, b2 = sc.case(syn, "s1r1").data, sc.case(syn, "s2r1").data
    sp = splice(a[:len(a)], a, 3)
    assert np.array_equal(sp, a)                                # a stream spliced with itself is itself
    assert sc.call_completing([10, 20, 30], 20) == 1 and sc.call_completing([10, 20, 30], 21) == 2
    assert len(b2)


def test_the_old_varrows_fixtures_leave_the_stepping_kernel_at_unit_0(pkg, oracle):
    """Why test_gpu_parity.py::test_streaming_tier_state_on_the_device_and_its_fall_back does not cover the hand-over: in
    every one of its VARROWS streams the first access unit is already of non-standard length, so the tier is on the
    batch-tier path before it holds any state -- no queue cut, no FIR history from the device, rows_before 0."""
    syn = pkg.synth
    SF = syn.SF
    fast = SF["CHAINED"] | SF["FIRRAND"] | SF["IIR"] | SF["PARAMBLOCKS"] | SF["MATRIXRAND"] | SF["MIDMATRIX"] | \
        SF["QSS"] | SF["OUTSHIFT"] | SF["VARBLOCK"] | SF["MIXBOOKS"] | SF["MIDRESTART"]
    for S in (1, 2):
        for feats in (fast | SF["VARROWS"], fast | SF["SYNCONLY"] | SF["VARROWS"]):
            for seed in range(4):
                cfg = syn.make_cfg(assignment=12 if S == 2 or seed % 2 == 0 else 1, rate_code=seed % 3, n_substreams=S,
                                   n_aus=36, profile=1, features=feats, restart_interval=[4, 3, 8, 5][seed])
                data, frames = syn.stream(cfg, 4100 + seed)
                first = data[:frame_offsets(data)[1]]
                _, r, st = oracle.decode(first, syn.channels(cfg.assignment), 400)
                assert st == 0 and r != syn.rows_per_au(cfg.rate_code), (S, seed)
