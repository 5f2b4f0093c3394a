"""The 2-channel presentation through the disc tier (include/dvd-audio-hip.h: dvda_hip_open_track_reader_with,
dvda_hip_set_presentation; tools/dvda2wav_hip.c --stereo): tracks of a two-substream title read with presentation=1
give the PCM of tests/presentation_model.py, as 2-channel frames, short tracks and windowed ones alike."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import presentation_model as pm
from tests.test_presentation_model import make_stream

pytestmark = pytest.mark.gpu


def _split_title(pkg, seed=3):
    """a plain two-substream 6-channel title of 96 units in three tracks (as _titles of tests/test_disc_api.py)"""
    disc = pkg.disc
    b, f = make_stream(pkg, 0, seed, n_aus=96)
    secs = disc.mlp_track_sectors(b)
    tracks = disc.split_tracks(secs, [len(secs) // 3, 2 * len(secs) // 3 + 1], [f // 3, f // 3, f - 2 * (f // 3)], 1)
    return b, f, tracks


def test_tracks_of_a_split_title_give_the_presentation(pkg, oracle):
    dd = pkg.discdec
    b, f, tracks = _split_title(pkg)
    want, frames, ost, k = pm.expect(b, oracle)
    assert ost == 0 and k == 2 and frames == f
    with tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [tracks])
        got = []
        for ki in (1, 2, 3):
            info = dd.read_track(ats, 1, 1, ki, chunk=1000, presentation=1)
            assert info["codec"] == "MLP" and info["channels"] == 2 and info["mask"] == 0x3 and info["bits"] == 24
            assert info["status"] & ~pkg.hipdec.ST_BENIGN == 0 and not info["windowed"]
            assert info["frames"] == len(info["pcm"]) > 0 and info["pcm"].shape[1] == 2
            got.append(info["pcm"])
            # the payload, packed behind an int32 decode and written by the decode kernels themselves
            packed = dd.read_track(ats, 1, 1, ki, wav=True, presentation=1)
            fused = dd.read_track(ats, 1, 1, ki, wav=True, fused=True, presentation=1)
            assert fused["wav_only"] and not packed["wav_only"] and fused["channels"] == packed["channels"] == 2
            assert fused["payload"] == packed["payload"] == oracle.wav_pack(info["pcm"].T, 24)
        assert np.array_equal(np.concatenate(got).T, want)
        # ... and the reader opened without it is the one it always was
        full, r, st = oracle.decode(b, 6, f)
        plain = np.concatenate([dd.read_track(ats, 1, 1, ki)["pcm"] for ki in (1, 2, 3)])
        assert st == 0 and np.array_equal(plain.T, full)


def test_windowed_read_of_a_chained_title(pkg, oracle):
    dd, disc = pkg.discdec, pkg.disc
    b, f = make_stream(pkg, "DISC|CHAINED|FIRRAND", 4, n_aus=1600)
    want, frames, ost, k = pm.expect(b, oracle)
    assert ost == 0 and k == 2 and frames == f
    secs = disc.mlp_track_sectors(b)
    assert len(secs) > 4 * 128
    with tempfile.TemporaryDirectory() as tmp:
        ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [], [f], 1)])
        whole = dd.read_track(ats, 1, 1, 1, presentation=1)           # the default window holds the track: one batch
        assert not whole["windowed"] and whole["channels"] == 2
        assert np.array_equal(whole["pcm"].T, want)
        old = os.environ.get("DVDA_WINDOW_SECTORS")
        os.environ["DVDA_WINDOW_SECTORS"] = "128"
        try:
            a = dd.read_track(ats, 1, 1, 1, chunk=3001, presentation=1)
            w = dd.read_track(ats, 1, 1, 1, wav=True, fused=True, pieces=True, presentation=1)
            # a windowed reader of the other presentation right behind it: the thread's cached context serves both
            six = dd.read_track(ats, 1, 1, 1, chunk=3001)
        finally:
            if old is None:
                del os.environ["DVDA_WINDOW_SECTORS"]
            else:
                os.environ["DVDA_WINDOW_SECTORS"] = old
        assert a["windowed"] and not a["failed"] and a["channels"] == 2 and a["mask"] == 0x3
        assert a["status"] & ~pkg.hipdec.ST_BENIGN == 0 and a["frames"] == len(a["pcm"]) == f
        assert np.array_equal(a["pcm"].T, want) and np.array_equal(a["pcm"], whole["pcm"])
        assert w["windowed"] and not w["failed"] and len(w["piece_sizes"]) >= 4
        assert w["payload"] == oracle.wav_pack(want, 24)
        full, r, st = oracle.decode(b, 6, f)
        assert st == 0 and six["windowed"] and six["channels"] == 6 and np.array_equal(six["pcm"].T, full)
        default = dd.read_track(ats, 1, 1, 1, presentation=0)
        assert default["channels"] == 6 and default["mask"] == 0x3F and np.array_equal(default["pcm"].T, full)


def test_tool_writes_stereo_files(pkg, oracle):
    tool = pkg._build.build_tool()
    b, f, tracks = _split_title(pkg)
    with tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [tracks])
        out = os.path.join(tmp, "out")
        os.makedirs(out)
        r = subprocess.run([tool, "-A", ats, "-d", out, "--stereo"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        files = sorted(os.listdir(out))
        assert files == ["track-01-01.wav", "track-01-02.wav", "track-01-03.wav"]
        for ki, name in enumerate(files, 1):
            data = open(os.path.join(out, name), "rb").read()
            want = pkg.discdec.read_track(ats, 1, 1, ki, wav=True, presentation=1)["payload"]
            assert data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt "
            assert int.from_bytes(data[22:24], "little") == 2 and int.from_bytes(data[40:44], "little") == 0x3
            assert int.from_bytes(data[34:36], "little") == 24 and int.from_bytes(data[64:68], "little") == len(want)
            assert data[68:] == want and len(want) > 0
        short = subprocess.run([tool, "-A", ats, "-d", out, "-2", "-t", "1"], capture_output=True, text=True, timeout=300)
        assert short.returncode == 0 and "2 channels" in short.stdout
