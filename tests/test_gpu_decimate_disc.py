"""The decimation through the disc tier (dvda_hip_set_decimate / dvda_hip_reader_decimated / dvda_hip_reader_source_rate,
discdec.read_track(decimate=...), dvda2wav_hip -r): a whole-track reader opened with the option IS the track of
ceil(F / D) frames at the lower rate -- its PCM, payload, frame count, rate, digest and the word-length reduction behind
it are tests/decimate_model of the same track read without the option.  Every comparison is exact."""
import ctypes
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from tests import decimate_model as dm
from tests import requant_model as rm
from tests.test_gpu_digest_disc import window_sectors

pytestmark = pytest.mark.gpu


def one_track(pkg, tmp, secs, frames, rate_code):
    return pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [], [frames], rate_code)])


def raw_pcm(pkg, seed, rate_code, n_sec, bps_code=2, assignment=12):
    """a raw-PCM track of n_sec sectors -> (its sectors, its PCM [frames, channels]); a run at the rails, so that the
    band-limited version overshoots"""
    disc = pkg.disc
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
    pcm = np.random.RandomState(seed).randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(per * n_sec, ch))
    for i, a in enumerate(range(100, 700, 60)):
        pcm[a:a + 60] = (1 << (bits - 1)) - 1 if i % 2 else -(1 << (bits - 1))
    return disc.pcm_track_sectors(pcm, bps_code, rate_code, assignment), pcm


@pytest.fixture(scope="module")
def discs(pkg):
    """three small discs of one track each: MLP at 96 kHz, raw PCM at 96 kHz, raw PCM at 48 kHz; per disc the AUDIO_TS
    path and the plain read of the track, made once"""
    syn, disc = pkg.synth, pkg.disc
    with tempfile.TemporaryDirectory() as tmp:
        out = {}
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=200), 91)
        out["mlp96"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), disc.mlp_track_sectors(b), f, 1)
        secs, pcm = raw_pcm(pkg, 601, 1, 60)
        out["pcm96"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), secs, len(pcm), 1)
        secs, pcm = raw_pcm(pkg, 602, 0, 40)
        out["pcm48"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), secs, len(pcm), 0)
        plain = {}
        for name, ats in out.items():
            plain[name] = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001)
            assert not plain[name]["windowed"] and "decimate" not in plain[name]
            plain[name]["pcm"].setflags(write=False)
        yield out, plain


def model(pkg, plain, ratio):
    src = np.ascontiguousarray(plain["pcm"].T)
    want, cl = dm.decimate_np(src, pkg.hipdec.decim_taps(ratio), ratio, plain["bits"])
    return want, dm.report(src.shape[1], want.shape[1], cl)


@pytest.mark.parametrize("name,codec", [("mlp96", "MLP"), ("pcm96", "PCM")])
def test_track_by_two(pkg, discs, name, codec):
    """read_track(decimate=2) equals the model of the plain read: frames, rate and report agree; as PCM and as the payload"""
    ats, plain = discs[0][name], discs[1][name]
    assert plain["codec"] == codec and plain["rate"] == 96000 and plain["bits"] == 24 and plain["channels"] == 6
    want, rep = model(pkg, plain, 2)
    assert want.shape[1] == (plain["frames"] + 1) // 2 and not np.array_equal(want, plain["pcm"].T[:, ::2])
    got = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001, decimate=2, digest=True)
    assert not got["windowed"] and got["codec"] == codec and got["bits"] == 24 and got["channels"] == 6
    assert (got["rate"], got["source_rate"], got["frames"]) == (48000, 96000, want.shape[1])
    assert got["decimate_state"] == 1 and got["decimate"] == rep
    assert np.array_equal(got["pcm"].T, want)
    pay = dm.payload(want, 24)
    assert (got["crc32"], got["crc32_bytes"]) == (zlib.crc32(pay), len(pay))
    for fused in (False, True):
        packed = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=fused, decimate=2)
        assert packed["payload"] == pay and not packed["wav_only"] and packed["rate"] == 48000
        assert packed["decimate"] == rep
    if name == "pcm96":
        assert sum(rep["clipped"]) > 0          # the run at the rails overshoots


@pytest.mark.parametrize("name", ["mlp96", "pcm96"])
def test_with_requant_and_digest(pkg, discs, name):
    """the word-length reduction works on the decimated track (its frame0 counts output frames), and the digest is that of
    the decimated, requantized payload"""
    ats, plain = discs[0][name], discs[1][name]
    dec, rep = model(pkg, plain, 2)
    want, cl = rm.requant_np(dec, 24, 16, rm.TPDF, 7, 0)
    pay = rm.payload(want, 16)
    got = pkg.discdec.read_track(ats, 1, 1, 1, decimate=2, requant=(16, rm.TPDF, 7), digest=True)
    assert (got["rate"], got["bits"], got["source_bits"], got["source_rate"]) == (48000, 16, 24, 96000)
    assert np.array_equal(got["pcm"].T, want) and got["decimate"] == rep
    assert got["requant"] == rm.report(want.shape[1], cl) and got["requant_states"] == (1, 1)
    assert (got["crc32"], got["crc32_bytes"]) == (zlib.crc32(pay), len(pay))
    packed = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=True, decimate=2, requant=(16, rm.TPDF, 7), digest=True)
    assert packed["payload"] == pay and packed["crc32"] == zlib.crc32(pay)


def test_rates_the_option_does_not_apply_to(pkg, discs):
    """a 48 kHz track comes out unchanged, with state 0; so does a 96 kHz track by 4 (24 kHz is not a rate)"""
    for name, ratio in (("pcm48", 2), ("pcm48", 4), ("mlp96", 4), ("pcm96", 4)):
        ats, plain = discs[0][name], discs[1][name]
        got = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001, decimate=ratio, digest=True)
        assert got["decimate_state"] == 0 and got["decimate"] is None
        assert got["rate"] == got["source_rate"] == plain["rate"] and got["frames"] == plain["frames"]
        assert np.array_equal(got["pcm"], plain["pcm"])
        pay = dm.payload(plain["pcm"].T, 24)
        assert got["crc32"] == zlib.crc32(pay)
    assert discs[1]["pcm48"]["rate"] == 48000


def test_by_four(pkg):
    """192 kHz by 4, and by 2"""
    secs, pcm = raw_pcm(pkg, 603, 2, 40, assignment=1)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, secs, len(pcm), 2)
        plain = pkg.discdec.read_track(ats, 1, 1, 1)
        assert plain["rate"] == 192000 and np.array_equal(plain["pcm"], pcm)
        for ratio in (4, 2):
            want, rep = model(pkg, plain, ratio)
            got = pkg.discdec.read_track(ats, 1, 1, 1, decimate=ratio)
            assert (got["rate"], got["source_rate"]) == (192000 // ratio, 192000)
            assert np.array_equal(got["pcm"].T, want) and got["decimate"] == rep


def test_windowed_track_and_bad_options_fail_the_open(pkg, discs):
    """a track the reader would take in windows: the open returns NULL; so do conceal mode and a ratio that does not exist"""
    syn, disc = pkg.synth, pkg.disc
    rt = pkg.discdec.read_track
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=400), 92)
    secs = disc.mlp_track_sectors(b)
    psecs, pcm = raw_pcm(pkg, 604, 1, 80)
    assert len(secs) > 64 and len(psecs) > 64
    with tempfile.TemporaryDirectory() as tmp:
        for s, n in ((secs, f), (psecs, len(pcm))):
            ats = one_track(pkg, tempfile.mkdtemp(dir=tmp), s, n, 1)
            with window_sectors(64):
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
                assert rt(ats, 1, 1, 1)["windowed"]
                with pytest.raises(RuntimeError, match="cannot be opened"):
                    rt(ats, 1, 1, 1, decimate=2)
                # by 4 the option does not apply to a 96 kHz track: read in windows as ever
                off = rt(ats, 1, 1, 1, decimate=4)
                assert off["windowed"] and off["decimate_state"] == 0 and off["rate"] == 96000
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
            assert rt(ats, 1, 1, 1, decimate=2)["rate"] == 48000
    ats = discs[0]["mlp96"]
    assert rt(ats, 1, 1, 1, decimate=2, conceal=False)["rate"] == 48000
    for kw in (dict(decimate=2, conceal=True), dict(decimate=3), dict(decimate=8), dict(decimate=1)):
        with pytest.raises(RuntimeError, match="cannot be opened"):
            rt(ats, 1, 1, 1, **kw)
    # the option is read when a reader is opened and nothing of it is left behind
    L = pkg.discdec.lib()
    d = L.dvda_open(ats.encode(), None)
    ts = L.dvda_open_titleset(d, 1)
    t = L.dvda_open_title(ts, 1)
    k = L.dvda_open_track(t, 1)
    r = L.dvda_open_track_reader(k)
    rep = pkg.hipdec.DecimReport(7, 7, (ctypes.c_uint64 * 8)(*[7] * 8))
    assert r and L.dvda_hip_reader_decimated(r, None) == 0
    assert L.dvda_hip_reader_decimated(r, ctypes.byref(rep)) == 0 and rep.as_dict() == dm.report(7, 7, [7] * 8)
    assert L.dvda_sample_rate(r) == L.dvda_hip_reader_source_rate(r) == 96000
    L.dvda_close_track_reader(r)
    L.dvda_close_track(k)
    L.dvda_close_title(t)
    L.dvda_close_titleset(ts)
    L.dvda_close(d)


def run_tool(tool, ats, out, args):
    r = subprocess.run([tool, "-A", ats, "-d", out, "--crc"] + args, capture_output=True, text=True, timeout=300)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    path = os.path.join(out, "track-01-01.wav")
    return r, lines, open(path, "rb").read() if os.path.exists(path) else None


def test_tool_rate_option(pkg, discs):
    """dvda2wav_hip -r 48000 -b 16: the header says 48 000 Hz and 16 bits, the data chunk is the model's payload, one
    DECIMATE line per track; a track that already runs at RATE is written as it is"""
    tool = pkg._build.build_tool()
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("mlp96", "pcm96"):
            ats, plain = discs[0][name], discs[1][name]
            dec, rep = model(pkg, plain, 2)
            want, cl = rm.requant_np(dec, 24, 16, rm.TPDF, 0, 0)
            pay = rm.payload(want, 16)
            r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["-r", "48000", "-b", "16"])
            assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
            channels, rate, _, align, bits = struct.unpack("<HIIHH", data[22:36])
            assert (channels, rate, align, bits) == (6, 48000, 12, 16)
            assert data[68:] == pay
            assert ["DECIMATE", "1", "1", "1", "96000", "48000", str(sum(rep["clipped"]))] in lines
            assert ["REQUANT", "1", "1", "1", "24", "16", str(sum(cl))] in lines
            assert ["CRC32", "1", "1", "1", "%08x" % zlib.crc32(pay), str(len(pay))] in lines
        ats, plain = discs[0]["mlp96"], discs[1]["mlp96"]
        r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["--rate=96000"])
        assert r.returncode == 0 and data[68:] == dm.payload(plain["pcm"].T, 24) and "Warning" not in r.stderr
        assert struct.unpack("<I", data[24:28])[0] == 96000
        assert ["DECIMATE", "1", "1", "1", "96000", "96000", "none"] in lines
        # 88 200 is the other family: written as it is, with a warning
        r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["-r", "88200"])
        assert r.returncode == 0 and data[68:] == dm.payload(plain["pcm"].T, 24) and "Warning" in r.stderr
        assert ["DECIMATE", "1", "1", "1", "96000", "96000", "none"] in lines
        for bad in (["-r", "24000"], ["-r", "48000", "--conceal"]):
            out = tempfile.mkdtemp(dir=tmp)
            r, _, _ = run_tool(tool, ats, out, bad)
            assert r.returncode != 0 and os.listdir(out) == []
        # a track read in windows fails only where it would have to be decimated: at RATE, or in the other family, it is
        # written as it is, in windows
        syn, disc = pkg.synth, pkg.disc
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=400), 92)
        psecs, pcm = raw_pcm(pkg, 604, 1, 80)
        long_mlp = one_track(pkg, tempfile.mkdtemp(dir=tmp), disc.mlp_track_sectors(b), f, 1)
        long_pcm = one_track(pkg, tempfile.mkdtemp(dir=tmp), psecs, len(pcm), 1)
        with window_sectors(64):
            plain = pkg.discdec.read_track(long_mlp, 1, 1, 1)
            assert plain["windowed"] and plain["rate"] == 96000
            for ats, pay, rate, warns in ((long_mlp, dm.payload(plain["pcm"].T, 24), "96000", False),
                                         (long_pcm, dm.payload(pcm.T, 24), "88200", True)):
                r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["-r", rate])
                assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
                assert "Read in windows" in r.stdout and ("Warning" in r.stderr) == warns
                assert struct.unpack("<I", data[24:28])[0] == 96000 and data[68:] == pay
                assert ["DECIMATE", "1", "1", "1", "96000", "96000", "none"] in lines
                assert ["CRC32", "1", "1", "1", "%08x" % zlib.crc32(pay), str(len(pay))] in lines
                out = tempfile.mkdtemp(dir=tmp)
                r, _, _ = run_tool(tool, ats, out, ["-r", "48000"])
                assert r.returncode != 0 and os.listdir(out) == [] and "read in windows" in r.stderr
            pkg.discdec.lib().dvda_hip_release_cached_buffers()
