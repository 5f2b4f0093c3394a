"""Conceal mode through the disc tier (dvda_hip_set_conceal / dvda_hip_reader_concealed, discdec.read_track(conceal=True),
dvda2wav_hip --conceal): a damaged MLP track comes out as tests/conceal_model.conceal composes the track's stream D
(tests/disc_damage.py: the bytes the demux yields, cut by the reader's rule) -- bit for bit, as int32 frames and in both
payload forms, with the model's spans; a clean track and a reader without the option are as they always were."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

from tests import conceal_model as cm
from tests import disc_damage as dd
from tests import levels_model as lm
from tests.test_conceal_disc_model import DAMAGES, KINDS, model_of, stream_of
from tests.test_gpu_digest_disc import window_sectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_track_disc(pkg, tmp, sectors, frames):
    return pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(sectors, [], [frames], 1)])


def model_spans(info):
    """the reader's spans in the model's terms: (first_frame, frames, byte_off, byte_end, LEADING | TRAILING)"""
    return [s[:4] + (s[5] & 3,) for s in info["concealed"]]


WINDOW = 64             # sectors, for the windowed reads (the whole-track reads use the default)


def check_readers(pkg, oracle, ats, track, want, want_spans, windowed=False):
    """every form a reader hands a track out in, against the composed expectation `want` [6, frames]; windowed: the same
    track read in windows of WINDOW sectors (the caller has set them) -- the spans are final only at the track's end"""
    hd = pkg.hipdec
    payload = oracle.wav_pack(want, 24)
    plain = pkg.discdec.read_track(ats, 1, 1, track, chunk=3001, conceal=True, digest=True, levels=True)
    assert plain["windowed"] == windowed and not plain.get("failed")
    assert plain["frames"] == want.shape[1] == len(plain["pcm"])
    assert np.array_equal(plain["pcm"].T, want)
    assert model_spans(plain) == want_spans and plain["concealed_states"] == ((0, 1) if windowed else (1, 1))
    assert all(s[4] for s in plain["concealed"]), "every span names its cause"
    if want_spans:
        assert plain["status"] & hd.ST_CONCEALED and not plain["status"] & ~(hd.ST_BENIGN | hd.ST_CONCEALED), hex(plain["status"])
    else:
        assert plain["status"] & ~hd.ST_BENIGN == 0
    # the reports are made of the composed track: the silence is in them
    assert plain["crc32"] == zlib.crc32(payload) and plain["crc32_bytes"] == len(payload)
    assert plain["levels"] == lm.levels(want, 24)
    packed = pkg.discdec.read_track(ats, 1, 1, track, wav=True, pieces=windowed, conceal=True, digest=True, levels=True)
    fused = pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=True, pieces=True, conceal=True, digest=True)
    assert fused["wav_only"] and not packed["wav_only"]
    assert packed["windowed"] == fused["windowed"] == windowed and not packed.get("failed") and not fused.get("failed")
    assert packed["crc32"] == zlib.crc32(payload) and packed["levels"] == plain["levels"]
    if windowed:
        assert len(fused["piece_sizes"]) >= 3 and len(packed["piece_sizes"]) >= 3
    assert packed["payload"] == payload and fused["payload"] == payload
    assert fused["crc32"] == zlib.crc32(payload)
    assert model_spans(packed) == want_spans and model_spans(fused) == want_spans
    assert fused["status"] == plain["status"] == packed["status"]
    return plain


def check_whole_and_windowed(pkg, oracle, ats, track, want, want_spans):
    """the track as one batch and in windows of WINDOW sectors: both are the model's composition, so the one equals the
    other byte for byte"""
    whole = check_readers(pkg, oracle, ats, track, want, want_spans)
    with window_sectors(WINDOW):
        pkg.discdec.lib().dvda_hip_release_cached_buffers()
        win = check_readers(pkg, oracle, ats, track, want, want_spans, windowed=True)
    assert np.array_equal(win["pcm"], whole["pcm"]) and model_spans(win) == model_spans(whole)
    return whole, win


@pytest.mark.parametrize("name", sorted(DAMAGES))
@pytest.mark.parametrize("S,feat", KINDS)
def test_damaged_tracks(pkg, oracle, S, feat, name):
    sectors, D, want, want_spans = model_of(pkg, oracle, S, feat, name)
    assert want_spans, "the damage must show in the model"
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, sectors, want.shape[1])
        assert len(sectors) > 4 * WINDOW
        check_whole_and_windowed(pkg, oracle, ats, 1, want, want_spans)


@pytest.mark.parametrize("where", ["first_sector", "first_sector_lost", "last_sector"])
def test_damage_at_the_ends_of_the_track(pkg, oracle, where):
    """a flipped byte in the track's first access unit (a LEADING span), in its last one (a TRAILING span), and a first
    sector that is lost whole: the stream then begins at the first major sync behind it -- a shorter track, no span"""
    b, frames, rpa = stream_of(pkg, 1, 0)
    n = -(-len(b) // dd.BODY)
    last_len = len(b) - (n - 1) * dd.BODY
    damage = dict(first_sector=dict(flips=((0, 200, 0x10),)), first_sector_lost=dict(lost=(0,)),
                  last_sector=dict(flips=((n - 1, last_len // 2, 0x10),)))[where]
    sectors, D = dd.damaged_track(pkg.disc, b, **damage)
    want, want_spans = cm.conceal(D, 6, rpa, oracle)
    assert 0 < want.shape[1] < frames
    assert [s[4] for s in want_spans] == dict(first_sector=[cm.LEADING], first_sector_lost=[], last_sector=[cm.TRAILING])[where]
    with tempfile.TemporaryDirectory() as tmp:
        check_whole_and_windowed(pkg, oracle, one_track_disc(pkg, tmp, sectors, frames), 1, want, want_spans)


@pytest.mark.parametrize("S,feat", KINDS[:2])
def test_a_long_run_of_garbage(pkg, oracle, S, feat):
    """5 x 64 sectors whose MLP bytes are random inside valid packets -- the demux accepts every one of them, the index
    finds whatever patterns the noise holds: one span, the track as long as the clean one"""
    b, frames, rpa = stream_of(pkg, S, feat)
    sectors, D = dd.damaged_track(pkg.disc, b, garbage=((40, 5 * 64, 7),))
    assert len(D) == len(b)
    want, want_spans = cm.conceal(D, 6, rpa, oracle)
    assert len(want_spans) == 1 and 0 < want_spans[0][1] < 65536 and want.shape[1] == frames
    with tempfile.TemporaryDirectory() as tmp:
        whole, win = check_whole_and_windowed(pkg, oracle, one_track_disc(pkg, tmp, sectors, frames), 1, want, want_spans)
        # bounded memory under damage: no cut is found inside the noise, and the reader does not let the waiting bytes
        # grow with it -- it holds no more than for the clean track read the same way, plus one window
        clean_sectors, _ = dd.damaged_track(pkg.disc, b)
        with window_sectors(WINDOW):
            pkg.discdec.lib().dvda_hip_release_cached_buffers()
            clean = pkg.discdec.read_track(one_track_disc(pkg, os.path.join(tmp, "clean"), clean_sectors, frames), 1, 1, 1,
                                           chunk=3001, conceal=True)
        assert clean["windowed"] and clean["concealed"] == []
        print("host_peak: damaged %d, clean %d, one window %d" % (win["host_peak"], clean["host_peak"], WINDOW * 2048))
        assert win["host_peak"] <= clean["host_peak"] + WINDOW * 2048


def test_malformed_first_sector_does_not_end_the_codec_probe(pkg, oracle):
    """a first sector whose pack header is broken: the probe goes on to the next sector, the demux refuses the sector"""
    b, frames, rpa = stream_of(pkg, 1, 0)
    sectors, bodies = dd.damaged_sectors(pkg.disc, b)
    sectors[0] = b"\x00\x00\x01\xBB" + sectors[0][4:]
    bodies[0] = None
    D = dd.track_stream(bodies, 0, len(bodies) - 1)
    want, want_spans = cm.conceal(D, 6, rpa, oracle)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, sectors, frames)
        info = pkg.discdec.read_track(ats, 1, 1, 1, conceal=True)
        assert np.array_equal(info["pcm"].T, want) and model_spans(info) == want_spans
        with pytest.raises(RuntimeError):
            pkg.discdec.read_track(ats, 1, 1, 1, conceal=False)


def test_damage_at_the_cut_of_a_two_track_title(pkg, oracle):
    """a flipped byte on each side of the cut between two tracks of one stream: each track's D follows the end-of-track
    rule (disc_damage.track_stream) -- the first track's runs into the second one's first sector, up to its first major
    sync, and ends in a TRAILING span; the second track begins at that sync -- and each reader delivers the model's
    composition of its own D"""
    b, frames, rpa = stream_of(pkg, 1, 0)
    cut = 200
    sectors, bodies = dd.damaged_sectors(pkg.disc, b, flips=((cut - 1, 1500, 0x10), (cut, 300, 0x10)))
    with tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(sectors, [cut], [frames // 2, frames - frames // 2], 1)])
        total = 0
        for track, (first, last) in enumerate([(0, cut - 1), (cut, len(bodies) - 1)], 1):
            D = dd.track_stream(bodies, first, last)
            want, want_spans = cm.conceal(D, 6, rpa, oracle)
            assert [s[4] for s in want_spans] == ([cm.TRAILING] if track == 1 else [])
            check_whole_and_windowed(pkg, oracle, ats, track, want, want_spans)
            total += want.shape[1]
        assert 0 < total < frames          # (what lies between the two tracks is neither's to fill)


def test_clean_track_reads_as_without_the_option(pkg, oracle):
    b, frames, rpa = stream_of(pkg, 2, "DISC|CHAINED")
    sectors, _ = dd.damaged_track(pkg.disc, b)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, sectors, frames)
        for kw in (dict(chunk=3001), dict(wav=True), dict(wav=True, fused=True, pieces=True)):
            off = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, conceal=False, **kw)
            on = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, conceal=True, **kw)
            assert on.pop("concealed") == [] and on.pop("concealed_states") == (1, 1)
            assert sorted(on) == sorted(off)
            for key in on:
                assert np.array_equal(on[key], off[key]), key
        assert off["frames"] == frames and off["status"] & ~pkg.hipdec.ST_BENIGN == 0
        # ... and in windows: the same windows, the same pieces (the memory peaks are sampled, not compared)
        with window_sectors(WINDOW):
            for kw in (dict(chunk=3001), dict(wav=True, pieces=True), dict(wav=True, fused=True, pieces=True)):
                off = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, conceal=False, **kw)
                on = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, conceal=True, **kw)
                assert on["windowed"] and off["windowed"] and not on["failed"]
                assert on.pop("concealed") == [] and on.pop("concealed_states") == (0, 1)
                assert sorted(on) == sorted(off)
                for key in on:
                    if key not in ("host_peak", "device_peak"):
                        assert np.array_equal(on[key], off[key]), key


def test_without_the_option_a_damaged_track_fails_as_before(pkg, oracle):
    sectors, D, want, want_spans = model_of(pkg, oracle, 1, 0, "scattered")
    L = pkg.discdec.lib()
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, sectors, want.shape[1])
        with pytest.raises(RuntimeError):
            pkg.discdec.read_track(ats, 1, 1, 1, conceal=False)
        # conceal mode of the 2-channel presentation: the batch tier has none, the reader does not open
        with pytest.raises(RuntimeError):
            pkg.discdec.read_track(ats, 1, 1, 1, conceal=True, presentation=1)
    # asked of a reader opened without it: -1
    b, frames, rpa = stream_of(pkg, 1, 0)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, pkg.disc.mlp_track_sectors(b), frames)
        d = L.dvda_open(ats.encode(), None)
        ts = L.dvda_open_titleset(d, 1)
        t = L.dvda_open_title(ts, 1)
        k = L.dvda_open_track(t, 1)
        L.dvda_hip_set_conceal(0)
        r = L.dvda_open_track_reader(k)
        n = ctypes.c_uint(7)
        assert r and L.dvda_hip_reader_concealed(r, None, 0, ctypes.byref(n)) == -1 and n.value == 7
        L.dvda_close_track_reader(r)
        L.dvda_close_track(k)
        L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
        L.dvda_close(d)


CHILD = """
import json, sys, zlib
sys.path.insert(0, sys.argv[1])
import libdvd_audio_amd as pkg
try:
    info = pkg.discdec.read_track(sys.argv[2], 1, 1, 1)
    print(json.dumps({"status": info["status"], "frames": info["frames"], "crc": zlib.crc32(info["pcm"].tobytes())}))
except RuntimeError:
    print(json.dumps({"status": None}))
"""


def test_environment_switch(pkg, oracle):
    """DVDA_CONCEAL=1 and no dvda_hip_set_conceal call on the thread: the reader conceals (a fresh process per setting:
    the option is the thread's); without the variable the damaged track does not open"""
    sectors, D, want, want_spans = model_of(pkg, oracle, 1, 0, "scattered")
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, sectors, want.shape[1])
        got = {}
        for value in ("1", None):
            env = {k: v for k, v in os.environ.items() if k != "DVDA_CONCEAL"}
            if value:
                env["DVDA_CONCEAL"] = value
            r = subprocess.run([sys.executable, "-c", CHILD, ROOT, ats], capture_output=True, text=True, env=env, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            got[value] = json.loads(r.stdout.strip().splitlines()[-1])
        assert got[None] == {"status": None}
        assert got["1"]["status"] & pkg.hipdec.ST_CONCEALED and got["1"]["frames"] == want.shape[1]
        assert got["1"]["crc"] == zlib.crc32(np.ascontiguousarray(want.T).tobytes())


def test_tool_conceal_option(pkg, oracle):
    """dvda2wav_hip --conceal writes the composed track and names the spans; without the option the run fails"""
    tool = pkg._build.build_tool()
    sectors, D, want, want_spans = model_of(pkg, oracle, 1, 0, "scattered")
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track_disc(pkg, tmp, sectors, want.shape[1])
        out = os.path.join(tmp, "out")
        os.makedirs(out)
        r = subprocess.run([tool, "-A", ats, "-d", out, "--conceal"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
        assert os.listdir(out) == ["track-01-01.wav"]
        data = open(os.path.join(out, "track-01-01.wav"), "rb").read()
        assert data[68:] == oracle.wav_pack(want, 24)
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("CONCEALED ")]
        assert all(ln[1:4] == ["1", "1", "1"] and int(ln[8], 16) for ln in lines)
        assert [tuple(int(v) for v in ln[4:8]) + (int(ln[9]) & 3,) for ln in lines] == want_spans
        plain = os.path.join(tmp, "plain")
        os.makedirs(plain)
        r = subprocess.run([tool, "-A", ats, "-d", plain], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "CONCEALED" not in r.stdout
