"""Conceal mode, CPU side: the rule's model (tests/conceal_model.py) against the oracle, and the new C ABI symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import conceal_model as cm
from tests.stream_tools import frame_offsets, is_major_sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KINDS = [(1, 0), (2, 0), (1, "CHAINED"), (2, "DISC|CHAINED"), (1, "NOCHECK")]


def make_stream(pkg, S, feat, seed=11, n_aus=48):
    """-> (bytes, PCM frames, rows per access unit): a recipe stream (feat 0) or one with the generator's features
    (names joined by |; CHAINED with random FIR taps at the restart points, as encoders write them)"""
    syn = pkg.synth
    f = 0
    for name in (feat.split("|") if feat else []):
        f |= syn.SF[name] | (syn.SF["FIRRAND"] if name == "CHAINED" else 0)
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=S, n_aus=n_aus, profile=1 if f else 0, features=f)
    b, frames = syn.stream(cfg, seed)
    return b, frames, syn.rows_per_au(1)


_stream = make_stream


@pytest.mark.parametrize("S,feat", KINDS)
def test_model_clean_is_the_oracle(pkg, oracle, S, feat):
    b, frames, rpa = _stream(pkg, S, feat)
    want, r, st = oracle.decode(b, 6, frames)
    assert st == 0 and r == frames
    got, spans = cm.conceal(b, 6, rpa, oracle)
    assert spans == []
    assert np.array_equal(got, want)


@pytest.mark.parametrize("S,feat", [k for k in KINDS if k[1] != "NOCHECK"])
def test_model_flip_stops_where_the_oracle_stops(pkg, oracle, S, feat):
    b, frames, rpa = _stream(pkg, S, feat)
    offs = frame_offsets(b)
    j = 19                                          # inside the third segment, not its major sync
    assert not is_major_sync(b, offs[j])
    d = b.copy()
    d[offs[j] + (offs[j + 1] - offs[j]) // 2] ^= 0x10
    whole, _, st = oracle.decode(d, 6, frames)
    assert st & cm.ORA_DAMAGE
    # the oracle's first failing unit: the shortest prefix it rejects ends with unit j
    assert oracle.decode(d[:offs[j + 1]], 6, frames)[2] & cm.ORA_DAMAGE
    assert not oracle.decode(d[:offs[j]], 6, frames)[2]
    rows = j * rpa
    R = cm.kept_ranges(d, 6, rpa, oracle)
    assert R[0][:3] == (0, offs[j], rows)           # kept: every unit in front of the damaged one
    # resumes at the next major sync behind it, decoded by a fresh decoder to the end
    nxt = next(o for o in offs if o > offs[j] and is_major_sync(b, o))
    assert R[1][0] == nxt and R[1][1] == len(d)
    pcm, spans = cm.conceal(d, 6, rpa, oracle)
    assert np.array_equal(pcm[:, :rows], whole[:, :rows])
    # the gap is the lost units' timing: the rest of the damaged segment
    assert spans == [(rows, (offs.index(nxt) - j) * rpa, offs[j], nxt, 0)]
    assert pcm.shape[1] == frames
    assert not pcm[:, rows:rows + spans[0][1]].any()


def test_model_nocheck_conceals_the_segment(pkg, oracle):
    b, frames, rpa = _stream(pkg, 1, "NOCHECK")
    offs = frame_offsets(b)
    seg0 = [o for o in offs if is_major_sync(b, o)]
    d, j = nocheck_flip(b, offs, oracle, frames)
    R = cm.kept_ranges(d, 6, rpa, oracle)
    start = max(o for o in seg0 if o <= offs[j])
    assert R[0][1] == start                         # the whole segment of the failing unit is concealed
    assert R[1][0] == min(o for o in seg0 if o > offs[j])


def nocheck_flip(b, offs, oracle, frames, first=17):
    """-> (copy of b with a flip the oracle rejects in a unit j >= first that carries no check data, j)"""
    for j in range(first, len(offs) - 9):
        p = offs[j]
        if is_major_sync(b, p) or (int(b[p + 4]) >> 5) & 1:
            continue                                # a major sync, or a unit with check data
        for k in range(p + 6, offs[j + 1] - 2):
            d = b.copy()
            d[k:k + 2] ^= 0xFF
            if oracle.decode(d[:offs[j + 1]], 6, frames)[2] & cm.ORA_DAMAGE:
                return d, j
    pytest.fail("no flip the oracle rejects in a unit without check data")


def test_model_gap_wraps_by_mean_bytes(pkg):
    # 90 000 frames lost at 2 bytes per frame: timing says 90 000 - 65 536, the bytes say one wrap more
    assert cm.gap_frames(180000, 90000 - 65536, 2.0) == 90000
    assert cm.gap_frames(480, 240, 2.0) == 240
    assert cm.gap_frames(0, 0, 0.0) == 0


def test_headers_declare_conceal_symbols():
    h = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    assert re.search(r"#define DVDA_ST_CONCEALED\s+\(1u << 30\)", h)
    for sym in ("dvda_mlp_hip_set_conceal", "dvda_mlp_hip_conceal_spans", "dvda_mlp_conceal_span"):
        assert sym in h
    # not benign: a caller has to ask for silence
    benign = re.search(r"#define DVDA_ST_BENIGN \((.*?)\)\n", h, re.S).group(1)
    assert "CONCEALED" not in benign


def test_library_exports_conceal_symbols(pkg):
    so = pkg._build.build_hip()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"dvda_mlp_hip_set_conceal", "dvda_mlp_hip_conceal_spans"} <= names
