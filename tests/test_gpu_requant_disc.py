"""The word-length reduction through the disc tier (dvda_hip_set_requantize / dvda_hip_reader_requantized,
discdec.read_track(requant=...), dvda2wav_hip -b): what a reader hands out -- PCM, payload, digest, level and energy
reports, its depth -- is tests/requant_model of the same track read without the option, whole-track and windowed alike.
Every comparison is exact."""
import ctypes
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from tests import energy_model as em
from tests import levels_model as lm
from tests import requant_model as rm
from tests.test_gpu_digest_disc import window_sectors

pytestmark = pytest.mark.gpu

B = 4800        # the energy report's grid in these tests


def one_track(pkg, tmp, secs, frames):
    return pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [], [frames], 1)])


def check_reader(info, want, cl, bits_out, states):
    """one read with the option on, every report beside it"""
    assert info["bits"] == bits_out and info["requant_states"] == states
    assert info["source_bits"] >= bits_out
    assert info["requant"] == rm.report(want.shape[1], cl)
    assert info["levels"] == lm.levels(want, bits_out) and info["energy"] == em.energy_fast(want, B)
    if bits_out in (16, 24):
        pay = rm.payload(want, bits_out)
        assert (info["crc32"], info["crc32_bytes"]) == (zlib.crc32(pay), len(pay))


def read_all_ways(pkg, ats, window, bits_in, rq, **kw):
    """the track without the option -> the model of it; then with the option: as one batch and in windows of `window`
    sectors, as PCM and as the payload (packed from int32, and from a reader opened for the payload alone)"""
    rt = pkg.discdec.read_track
    bits_out, mode, seed = rq
    plain = rt(ats, 1, 1, 1, chunk=3001, **kw)
    assert plain["bits"] == bits_in and not plain["windowed"] and "requant" not in plain
    want, cl = rm.requant_np(np.ascontiguousarray(plain["pcm"].T), bits_in, bits_out, mode, seed, 0)
    assert not np.array_equal(want, plain["pcm"].T)
    on = dict(requant=rq, digest=True, levels=True, energy=B, **kw)
    whole = rt(ats, 1, 1, 1, chunk=3001, **on)
    assert not whole["windowed"] and np.array_equal(whole["pcm"].T, want)
    check_reader(whole, want, cl, bits_out, (1, 1))
    pay = rm.payload(want, bits_out)
    for fused in (False, True):
        packed = rt(ats, 1, 1, 1, wav=True, fused=fused, **on)
        assert packed["payload"] == pay and not packed["wav_only"]
        check_reader(packed, want, cl, bits_out, (1, 1))
    with window_sectors(window):
        pkg.discdec.lib().dvda_hip_release_cached_buffers()
        win = rt(ats, 1, 1, 1, chunk=3001, **on)
        assert win["windowed"] and not win.get("failed") and np.array_equal(win["pcm"].T, want)
        check_reader(win, want, cl, bits_out, (0, 1))
        for fused in (False, True):
            packed = rt(ats, 1, 1, 1, wav=True, fused=fused, pieces=True, **on)
            assert packed["windowed"] and len(packed["piece_sizes"]) >= 3 and packed["payload"] == pay
            check_reader(packed, want, cl, bits_out, (0, 1))
        # the windowed read without the option is what it was
        off = rt(ats, 1, 1, 1, chunk=3001, digest=True, **kw)
        assert off["windowed"] and np.array_equal(off["pcm"], plain["pcm"]) and off["bits"] == bits_in
        pkg.discdec.lib().dvda_hip_release_cached_buffers()
    return plain, want, cl


def test_mlp_track(pkg):
    syn, disc = pkg.synth, pkg.disc
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=1600), 77)
    secs = disc.mlp_track_sectors(b)
    assert len(secs) > 4 * 128
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, secs, f)
        plain, want, cl = read_all_ways(pkg, ats, 128, 24, (16, rm.TPDF, 5))
        assert plain["codec"] == "MLP" and plain["channels"] == 6 and plain["frames"] == f
        # 20 bits: no payload and no digest at that depth; the PCM and the other reports as ever
        want20, cl20 = rm.requant_np(np.ascontiguousarray(plain["pcm"].T), 24, 20, rm.ROUND, 0, 0)
        r20 = pkg.discdec.read_track(ats, 1, 1, 1, requant=(20, rm.ROUND, 0), digest=True, levels=True, energy=B)
        assert np.array_equal(r20["pcm"].T, want20) and r20["crc32"] is None
        check_reader(r20, want20, cl20, 20, (1, 1))
        # 24 bits on a 24-bit track: a pure clamp
        r24 = pkg.discdec.read_track(ats, 1, 1, 1, requant=(24, rm.TPDF, 9), levels=True)
        clamp, cl24 = rm.requant_np(np.ascontiguousarray(plain["pcm"].T), 24, 24, rm.TPDF, 9, 0)
        assert np.array_equal(r24["pcm"].T, clamp) and r24["requant"] == rm.report(f, cl24) and r24["bits"] == 24
        assert r24["levels"]["over"] == [0] * 8


@pytest.mark.parametrize("mode", [rm.TRUNCATE, rm.TPDF])
def test_raw_pcm_track(pkg, mode):
    disc = pkg.disc
    bps_code, assignment = 2, 12
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    n_sec = 400
    per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
    frames = per * n_sec
    pcm = np.random.RandomState(502).randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(frames, ch))
    pcm[5:50] = (1 << 23) - 1               # at the rail: truncated it fits 16 bits, rounded up it does not
    secs = disc.pcm_track_sectors(pcm, bps_code, 1, assignment)
    assert len(secs) == n_sec > 4 * 64
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, secs, frames)
        plain, want, cl = read_all_ways(pkg, ats, 64, 24, (16, mode, 0xFEEDFACE))
        assert plain["codec"] == "PCM" and np.array_equal(plain["pcm"], pcm)
        assert (sum(cl) > 0) == (mode == rm.TPDF)


def test_presentation(pkg):
    """the 2-channel presentation of a two-substream track falls out of the rule"""
    syn, disc = pkg.synth, pkg.disc
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=1600), 79)
    secs = disc.mlp_track_sectors(b)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, secs, f)
        plain, want, cl = read_all_ways(pkg, ats, 128, 24, (16, rm.TPDF, 1), presentation=1)
        assert plain["channels"] == 2 and want.shape == (2, f)


def test_sixteen_bit_track(pkg):
    """at bits_out == 16 a 16-bit track is clamped and nothing else: unchanged, nothing clipped; at 20 and 24 the option
    is off for the reader, which hands the track out as it is"""
    disc = pkg.disc
    bps_code, assignment = 0, 1
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    n_sec = 300
    per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
    frames = per * n_sec
    pcm = np.random.RandomState(503).randint(-(1 << 15), 1 << 15, size=(frames, ch))
    secs = disc.pcm_track_sectors(pcm, bps_code, 1, assignment)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, secs, frames)
        rt = pkg.discdec.read_track
        plain = rt(ats, 1, 1, 1, digest=True)
        assert plain["bits"] == 16 and np.array_equal(plain["pcm"], pcm)
        for window in (None, 64):
            with window_sectors(window or 1 << 20):
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
                same = rt(ats, 1, 1, 1, requant=(16, rm.TPDF, 3), digest=True)
                assert same["windowed"] == bool(window) and np.array_equal(same["pcm"], pcm) and same["bits"] == 16
                assert same["requant"] == rm.report(frames, [0] * 8) and same["requant_states"][1] == 1
                assert same["crc32"] == plain["crc32"]
                for bits_out in (20, 24):
                    off = rt(ats, 1, 1, 1, requant=(bits_out, rm.TPDF, 3), digest=True)
                    assert off["bits"] == 16 and np.array_equal(off["pcm"], pcm) and off["crc32"] == plain["crc32"]
                    assert off["requant"] is None and off["requant_states"] == (-1, -1)
                    assert off["source_bits"] == 16
                    pay = rt(ats, 1, 1, 1, wav=True, fused=True, requant=(bits_out, rm.TPDF, 3))
                    assert pay["payload"] == rm.payload(pcm.T, 16)
                pkg.discdec.lib().dvda_hip_release_cached_buffers()


def test_conceal_mode_and_bad_options_fail_the_open(pkg):
    syn, disc = pkg.synth, pkg.disc
    b, f = syn.stream(syn.make_cfg(assignment=1, rate_code=1, n_substreams=1, n_aus=100), 80)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, disc.mlp_track_sectors(b), f)
        rt = pkg.discdec.read_track
        assert rt(ats, 1, 1, 1, requant=(16, rm.TPDF, 0), conceal=False)["bits"] == 16
        for kw in (dict(requant=(16, rm.TPDF, 0), conceal=True), dict(requant=(18, rm.TPDF, 0)), dict(requant=(16, 3, 0))):
            with pytest.raises(RuntimeError, match="cannot be opened"):
                rt(ats, 1, 1, 1, **kw)
        # the option is read when a reader is opened and nothing of it is left behind
        plain = rt(ats, 1, 1, 1)
        assert plain["bits"] == 24 and "requant" not in plain
        L = pkg.discdec.lib()
        d = L.dvda_open(ats.encode(), None)
        ts = L.dvda_open_titleset(d, 1)
        t = L.dvda_open_title(ts, 1)
        k = L.dvda_open_track(t, 1)
        r = L.dvda_open_track_reader(k)
        rep = pkg.hipdec.RequantReport(7, (ctypes.c_uint64 * 8)(*[7] * 8))
        assert r and L.dvda_hip_reader_requantized(r, None) == -1
        assert L.dvda_hip_reader_requantized(r, ctypes.byref(rep)) == -1 and rep.as_dict() == rm.report(7, [7] * 8)
        L.dvda_close_track_reader(r)
        L.dvda_close_track(k)
        L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
        L.dvda_close(d)


def test_tool_bits_option(pkg):
    """dvda2wav_hip -b 16: the header says 16 bits, the data chunk is the model's payload, one REQUANT line per track"""
    syn, disc = pkg.synth, pkg.disc
    tool = pkg._build.build_tool()
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=200), 81)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, disc.mlp_track_sectors(b), f)
        plain = pkg.discdec.read_track(ats, 1, 1, 1)
        src = np.ascontiguousarray(plain["pcm"].T)
        for args, mode, seed in ((["-b", "16"], rm.TPDF, 0), (["--bits=16", "--dither=tpdf", "--seed=12345"], rm.TPDF, 12345),
                                 (["-b", "16", "--dither=round"], rm.ROUND, 0), (["-b", "16", "--dither=none"], rm.TRUNCATE, 0)):
            out = tempfile.mkdtemp(dir=tmp)
            r = subprocess.run([tool, "-A", ats, "-d", out, "--crc"] + args, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
            data = open(os.path.join(out, "track-01-01.wav"), "rb").read()
            want, cl = rm.requant_np(src, 24, 16, mode, seed, 0)
            pay = rm.payload(want, 16)
            channels, rate, _, align, bits = struct.unpack("<HIIHH", data[22:36])
            assert (channels, rate, align, bits) == (6, 96000, 12, 16)
            assert data[68:] == pay
            lines = [ln.split() for ln in r.stdout.splitlines()]
            assert ["REQUANT", "1", "1", "1", "24", "16", str(sum(cl))] in lines
            assert ["CRC32", "1", "1", "1", "%08x" % zlib.crc32(pay), str(len(pay))] in lines
        # 24 bits on the 24-bit track: the file as without the option, but clamped (nothing to clamp here)
        out = tempfile.mkdtemp(dir=tmp)
        r = subprocess.run([tool, "-A", ats, "-d", out, "-b", "24"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and open(os.path.join(out, "track-01-01.wav"), "rb").read()[68:] == rm.payload(src, 24)
        assert ["REQUANT", "1", "1", "1", "24", "24", "0"] in [ln.split() for ln in r.stdout.splitlines()]
        for bad in (["-b", "20"], ["-b", "16", "--conceal"], ["-b", "16", "--dither=shaped"]):
            out = tempfile.mkdtemp(dir=tmp)
            r = subprocess.run([tool, "-A", ats, "-d", out] + bad, capture_output=True, text=True, timeout=300)
            assert r.returncode != 0 and os.listdir(out) == []
