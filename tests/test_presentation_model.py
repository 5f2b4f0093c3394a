"""The presentation rule, CPU side: the model (tests/presentation_model.py) against the oracle and the compiled
reference, and the new C ABI symbols.  The model is the yardstick of tests/test_gpu_presentation*.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import oracle_lib
from tests import presentation_model as pm
from tests.stream_tools import frame_offsets, is_major_sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRES_DIGESTS = os.path.join(ROOT, "tests", "golden", "presentation_digests.json")

FEATS = [0, "CHAINED", "DISC|CHAINED", "DISC|CHAINED|FIRRAND|MIXBOOKS", "CHAINED|NOISE|OUTSHIFT", "IIR|QSS",
         "SYNCONLY|CHAINED", "CHECKQUIRK|EXTRAWORD", "SF_ALL"]
# (assignment, channels of substream 0): every split of 1, 2, 3 and 5 channels under assignments 6, 12 and 20
SPLITS = [(12, 2), (6, 1), (20, 3), (12, 5), (6, 2), (20, 1), (12, 3), (20, 5), (6, 3), (12, 1), (20, 2)]
CONFIGS = [(feat, seed, SPLITS[(3 * i + seed) % len(SPLITS)]) for i, feat in enumerate(FEATS) for seed in (0, 1, 2)]
CONFIGS += [(0, 3, (12, 5)), ("CHAINED", 3, (20, 5)), ("DISC|CHAINED", 3, (6, 3))]
assert len(CONFIGS) == 30


def features(pkg, feat):
    syn = pkg.synth
    if feat == "SF_ALL":
        return syn.SF_ALL
    f = 0
    for name in (feat.split("|") if feat else []):
        f |= syn.SF[name] | (syn.SF["FIRRAND"] if name == "CHAINED" else 0)
    return f


def make_stream(pkg, feat, seed=11, assignment=12, ss0=2, S=2, n_aus=48):
    """-> (bytes, PCM frames of the full decode): 48 access units, restart interval 8, rate code 1"""
    syn = pkg.synth
    f = features(pkg, feat)
    kw = dict(ss0_channels=ss0) if S == 2 else {}
    cfg = syn.make_cfg(assignment=assignment, rate_code=1, n_substreams=S, n_aus=n_aus, profile=1 if f else 0,
                       features=f, restart_interval=8, **kw)
    return syn.stream(cfg, 7000 + 13 * seed)


def ss1_flip(b, unit, sub):
    """-> copy of b with one bit flipped in the middle of substream `sub`'s body of access unit `unit`"""
    offs = frame_offsets(b)
    p = offs[unit]
    fe = offs[unit + 1]
    q = p + (32 if is_major_sync(b, p) else 4)
    ends = []
    for s in range(2):
        w = (int(b[q]) << 8) | int(b[q + 1])
        ends.append((w & 0xFFF) * 2)
        q += 4 if w & 0x8000 else 2
    lo, hi = (0, ends[0]) if sub == 0 else (ends[0], ends[1])
    assert q + hi <= fe and hi - lo > 8
    d = b.copy()
    d[q + (lo + hi) // 2] ^= 0x10
    return d


@pytest.mark.parametrize("feat,seed,split", CONFIGS)
def test_stripped_stream_decodes_clean_and_differs(pkg, oracle, feat, seed, split, monkeypatch):
    syn = pkg.synth
    asg, ss0 = split
    b, frames = make_stream(pkg, feat, seed, asg, ss0)
    nch = syn.channels(asg)
    full, r, st = oracle.decode(b, nch, frames)
    assert st == 0 and r == frames
    s, k, pst = pm.strip(b)
    assert pst == 0 and k == ss0
    assert pm.substreams_of(s) == 1 and int(s[11]) & 0x1F == pm.IDENTITY_ASSIGNMENT[k]
    assert len(s) < len(b) and frame_offsets(s)[-1] < len(s) and len(frame_offsets(s)) == len(frame_offsets(b))
    pcm, pr, ost, pk = pm.expect(b, oracle)
    assert ost == 0 and pr == frames and pk == k and pcm.shape == (k, frames)
    # the mix is not the full decode's first k channels (RIFF order of the source's assignment)
    assert not np.array_equal(pcm, full[:k])
    # the restatement agrees with the compiled reference on the stripped stream (live where it is built, else by digest)
    monkeypatch.setattr(oracle_lib, "REF_DIGESTS", PRES_DIGESTS)
    key = "presentation_%s_%d_%d_%d" % (feat or "plain", seed, asg, ss0)
    assert oracle_lib.same_as_reference(
        key, (pcm, pr), lambda: oracle_lib.Reference().decode(s, pm.IDENTITY_ASSIGNMENT[k], 1, 2, frames))


def test_two_of_six_keeps_a_third_of_the_bytes(pkg):
    for feat in (0, "CHAINED", "DISC|CHAINED"):
        b, _ = make_stream(pkg, feat, 1)
        s, k, _ = pm.strip(b)
        assert k == 2 and 0.25 < len(s) / len(b) < 0.45


@pytest.mark.parametrize("asg", [12, 1])
def test_one_substream_strips_to_itself(pkg, oracle, asg):
    b, frames = make_stream(pkg, "CHAINED", 2, asg, S=1)
    s, k, st = pm.strip(b)
    assert st == 0 and k is None and np.array_equal(s, b)
    nch = pkg.synth.channels(asg)
    pcm, r, ost, pk = pm.expect(b, oracle, nch)
    want, wr, wst = oracle.decode(b, nch, frames)
    assert (r, ost, pk) == (wr, wst, nch) and np.array_equal(pcm, want)


def test_damage_in_substream_1_leaves_the_presentation_alone(pkg, oracle):
    b, frames = make_stream(pkg, "CHAINED", 0)
    d = ss1_flip(b, 19, 1)
    assert oracle.decode(d, 6, frames)[2] != 0
    assert np.array_equal(pm.strip(d)[0], pm.strip(b)[0])
    d0 = ss1_flip(b, 19, 0)
    assert pm.expect(d0, oracle)[2] != 0


def test_first_unit_without_restart_header_is_outside_the_envelope(pkg):
    b, _ = make_stream(pkg, 0, 0)
    cut = b[frame_offsets(b)[1]:].copy()          # starts with a unit that is no major sync: not a stream at all
    assert pm.strip(cut)[1] is None
    d = b.copy()
    q = 32 + 4                                    # first unit: major sync, two directory words
    assert (int(d[q]) & 0xC0) == 0xC0
    d[q] &= 0x7F
    assert pm.strip(d)[2] == pm.ST_ENVELOPE


def test_header_declares_presentation_symbols():
    h = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    assert re.search(r"#define DVDA_PRESENT_FULL\s+0u", h) and re.search(r"#define DVDA_PRESENT_SUBSTREAM0\s+1u", h)
    assert "dvda_mlp_hip_set_presentation" in h
    d = open(os.path.join(ROOT, "include", "dvd-audio-hip.h")).read()
    assert "dvda_hip_set_presentation" in d and "dvda_hip_open_track_reader_with" in d


def test_library_exports_presentation_symbols(pkg):
    so = pkg._build.build_hip()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "dvda_mlp_hip_set_presentation" in names
    assert "dvda_mlp_hip_set_presentation" in pkg.hipdec.EXPORTS
