"""The resampler through the disc tier (dvda_hip_set_resample / dvda_hip_reader_resampled, discdec.read_track(resample=
44100), dvda2wav_hip -r 44100 --resample): a whole-track reader opened with the option IS the 44.1 kHz track -- its PCM,
payload, frame count, rate, digest and the word-length reduction behind it are the composed models (tests/decimate_model
where the rate asks for it, then tests/resample_model) of the same track read without the option.  Every comparison is
exact."""
import ctypes
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from tests import decimate_model as dm
from tests import requant_model as qm
from tests import resample_model as rm
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
    """small discs of one track each: MLP at 96 kHz, raw PCM at 48 kHz, raw PCM at 44.1 kHz; per disc the AUDIO_TS path and
    the plain read of the track, made once"""
    syn, disc = pkg.synth, pkg.disc
    with tempfile.TemporaryDirectory() as tmp:
        out = {}
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=200), 93)
        out["mlp96"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), disc.mlp_track_sectors(b), f, 1)
        secs, pcm = raw_pcm(pkg, 611, 0, 40)
        out["pcm48"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), secs, len(pcm), 0)
        secs, pcm = raw_pcm(pkg, 612, 8, 30)
        out["pcm44"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), secs, len(pcm), 8)
        plain = {}
        for name, ats in out.items():
            plain[name] = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001)
            assert not plain[name]["windowed"] and "resample" not in plain[name]
            plain[name]["pcm"].setflags(write=False)
        yield out, plain


def model(pkg, plain):
    """-> (the 44.1 kHz track, the resampler's report, the report of the decimation in front of it or None)"""
    hd = pkg.hipdec
    src = np.ascontiguousarray(plain["pcm"].T)
    D = plain["rate"] // 48000
    rep_d = None
    if D > 1:
        mid, cl = dm.decimate_np(src, hd.decim_taps(D), D, plain["bits"])
        rep_d = dm.report(src.shape[1], mid.shape[1], cl)
        src = mid
    want, cl = rm.resample_np(src, hd.resample_taps(), plain["bits"])
    return want, rm.report(src.shape[1], want.shape[1], cl), rep_d


@pytest.mark.parametrize("name,codec,rate", [("mlp96", "MLP", 96000), ("pcm48", "PCM", 48000)])
def test_track_at_44100(pkg, discs, name, codec, rate):
    """read_track(resample=44100) equals the composed model of the plain read: frames, rate and reports agree; as PCM and
    as the payload"""
    ats, plain = discs[0][name], discs[1][name]
    assert plain["codec"] == codec and plain["rate"] == rate and plain["bits"] == 24 and plain["channels"] == 6
    want, rep, rep_d = model(pkg, plain)
    assert want.shape[1] == -(-147 * -(-plain["frames"] // (rate // 48000)) // 160)
    got = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001, resample=44100, digest=True)
    assert not got["windowed"] and got["codec"] == codec and got["bits"] == 24 and got["channels"] == 6
    assert (got["rate"], got["source_rate"], got["frames"]) == (44100, rate, want.shape[1])
    assert got["resample_state"] == 1 and got["resample"] == rep and got["resample_decimate"] == rep_d
    assert (rep_d is None) == (rate == 48000)
    assert np.array_equal(got["pcm"].T, want)
    pay = rm.payload(want, 24)
    assert (got["crc32"], got["crc32_bytes"]) == (zlib.crc32(pay), len(pay))
    for fused in (False, True):
        packed = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=fused, resample=44100)
        assert packed["payload"] == pay and not packed["wav_only"] and packed["rate"] == 44100
        assert packed["resample"] == rep
    if name == "pcm48":
        assert sum(rep["clipped"]) > 0          # the run at the rails overshoots


@pytest.mark.parametrize("name", ["mlp96", "pcm48"])
def test_with_requant_and_digest(pkg, discs, name):
    """the word-length reduction works on the 44.1 kHz track (its frame0 counts output frames), and the digest is that of
    the resampled, requantized payload"""
    ats, plain = discs[0][name], discs[1][name]
    res, rep, _ = model(pkg, plain)
    want, cl = qm.requant_np(res, 24, 16, qm.TPDF, 7, 0)
    pay = qm.payload(want, 16)
    got = pkg.discdec.read_track(ats, 1, 1, 1, resample=44100, requant=(16, qm.TPDF, 7), digest=True)
    assert (got["rate"], got["bits"], got["source_bits"], got["source_rate"]) == (44100, 16, 24, plain["rate"])
    assert np.array_equal(got["pcm"].T, want) and got["resample"] == rep
    assert got["requant"] == qm.report(want.shape[1], cl) and got["requant_states"] == (1, 1)
    assert (got["crc32"], got["crc32_bytes"]) == (zlib.crc32(pay), len(pay))
    packed = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=True, resample=44100, requant=(16, qm.TPDF, 7), digest=True)
    assert packed["payload"] == pay and packed["crc32"] == zlib.crc32(pay)


def test_a_track_of_the_other_family_is_unchanged(pkg, discs):
    ats, plain = discs[0]["pcm44"], discs[1]["pcm44"]
    assert plain["rate"] == 44100
    got = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001, resample=44100, digest=True)
    assert got["resample_state"] == 0 and got["resample"] is None and got["resample_decimate"] is None
    assert got["rate"] == got["source_rate"] == 44100 and got["frames"] == plain["frames"]
    assert np.array_equal(got["pcm"], plain["pcm"])
    assert got["crc32"] == zlib.crc32(rm.payload(plain["pcm"].T, 24))


def test_192_khz(pkg):
    """by 4, then resampled"""
    secs, pcm = raw_pcm(pkg, 613, 2, 40, assignment=1)
    with tempfile.TemporaryDirectory() as tmp:
        ats = one_track(pkg, tmp, secs, len(pcm), 2)
        plain = pkg.discdec.read_track(ats, 1, 1, 1)
        assert plain["rate"] == 192000 and np.array_equal(plain["pcm"], pcm)
        want, rep, rep_d = model(pkg, plain)
        got = pkg.discdec.read_track(ats, 1, 1, 1, resample=44100)
        assert (got["rate"], got["source_rate"]) == (44100, 192000)
        assert np.array_equal(got["pcm"].T, want) and got["resample"] == rep and got["resample_decimate"] == rep_d


def test_refused_opens(pkg, discs):
    """a track the reader would take in windows, conceal mode, both options at once, a wrong rate: the open returns NULL"""
    syn, disc = pkg.synth, pkg.disc
    rt = pkg.discdec.read_track
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=400), 94)
    secs = disc.mlp_track_sectors(b)
    psecs, pcm = raw_pcm(pkg, 614, 0, 80)
    assert len(secs) > 64 and len(psecs) > 64
    with tempfile.TemporaryDirectory() as tmp:
        for s, n, rc in ((secs, f, 1), (psecs, len(pcm), 0)):
            ats = one_track(pkg, tempfile.mkdtemp(dir=tmp), s, n, rc)
            with window_sectors(64):
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
                assert rt(ats, 1, 1, 1)["windowed"]
                with pytest.raises(RuntimeError, match="cannot be opened"):
                    rt(ats, 1, 1, 1, resample=44100)
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
            assert rt(ats, 1, 1, 1, resample=44100)["rate"] == 44100
    ats = discs[0]["mlp96"]
    assert rt(ats, 1, 1, 1, resample=44100, conceal=False)["rate"] == 44100
    for kw in (dict(resample=44100, conceal=True), dict(resample=44100, decimate=2), dict(resample=48000), dict(resample=1),
               dict(resample=22050), dict(resample=88200)):
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
    assert r and L.dvda_hip_reader_resampled(r, None) == 0 and L.dvda_hip_reader_resampled(None, None) == 0
    assert L.dvda_hip_reader_resampled(r, ctypes.byref(rep)) == 0 and rep.as_dict() == rm.report(7, 7, [7] * 8)
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


def test_tool_resample_option(pkg, discs):
    """dvda2wav_hip -r 44100 --resample -b 16: the header says 44 100 Hz and 16 bits, the data chunk is the model's
    payload, one RESAMPLE line per track; a track that already runs at 44.1 kHz is written as it is"""
    tool = pkg._build.build_tool()
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("mlp96", "pcm48"):
            ats, plain = discs[0][name], discs[1][name]
            res, rep, rep_d = model(pkg, plain)
            want, cl = qm.requant_np(res, 24, 16, qm.TPDF, 0, 0)
            pay = qm.payload(want, 16)
            r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["-r", "44100", "--resample", "-b", "16"])
            assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
            assert "Warning" not in r.stderr
            channels, rate, _, align, bits = struct.unpack("<HIIHH", data[22:36])
            assert (channels, rate, align, bits) == (6, 44100, 12, 16)
            assert data[68:] == pay
            clipped = sum(rep["clipped"]) + (sum(rep_d["clipped"]) if rep_d else 0)
            assert ["RESAMPLE", "1", "1", "1", str(plain["rate"]), "44100", str(clipped)] in lines
            assert ["REQUANT", "1", "1", "1", "24", "16", str(sum(cl))] in lines
            assert ["CRC32", "1", "1", "1", "%08x" % zlib.crc32(pay), str(len(pay))] in lines
        ats, plain = discs[0]["pcm44"], discs[1]["pcm44"]
        r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["-r", "44100", "--resample"])
        assert r.returncode == 0 and data[68:] == rm.payload(plain["pcm"].T, 24) and "Warning" not in r.stderr
        assert struct.unpack("<I", data[24:28])[0] == 44100
        assert ["RESAMPLE", "1", "1", "1", "44100", "44100", "none"] in lines
        # without the flag the tool is as it was: the track as it is, with a warning
        ats, plain = discs[0]["pcm48"], discs[1]["pcm48"]
        r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["-r", "44100"])
        assert r.returncode == 0 and data[68:] == rm.payload(plain["pcm"].T, 24) and "Warning" in r.stderr
        assert ["DECIMATE", "1", "1", "1", "48000", "48000", "none"] in lines and not any(ln[:1] == ["RESAMPLE"] for ln in lines)
        for bad in (["--resample"], ["-r", "48000", "--resample"], ["-r", "44100", "--resample", "--conceal"]):
            out = tempfile.mkdtemp(dir=tmp)
            r, _, _ = run_tool(tool, ats, out, bad)
            assert r.returncode != 0 and os.listdir(out) == []
