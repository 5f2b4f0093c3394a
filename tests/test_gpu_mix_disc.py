"""The channel mix through the disc tier (dvda_hip_set_downmix / dvda_hip_reader_downmixed / dvda_hip_reader_source_channels,
discdec.read_track(downmix=), dvda2wav_hip --downmix): a whole-track reader opened with the option IS the 1- or 2-channel
track -- its PCM, payload, channel count, mask, digest and the decimation, the resampler and the word-length reduction
behind it are the models (tests/mix_model first, then tests/decimate_model / tests/resample_model, then
tests/requant_model: every stage rounds and clamps, so the order is part of the contract) of the same track read
without the option.  Every comparison is exact."""
import ctypes
import os
import struct
import tempfile
import zlib

import numpy as np
import pytest

from tests import decimate_model as dm
from tests import mix_model as mm
from tests import requant_model as qm
from tests import resample_model as rm
from tests.test_gpu_digest_disc import window_sectors
from tests.test_gpu_resample_disc import one_track, raw_pcm, run_tool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def discs(pkg):
    """small discs of one track each: a 6-channel one-substream MLP track at 96 kHz, a 6-channel raw-PCM track at 48 kHz, a
    two-substream MLP track; per disc the AUDIO_TS path and the plain read of the track, made once"""
    syn, disc = pkg.synth, pkg.disc
    with tempfile.TemporaryDirectory() as tmp:
        out = {}
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=120), 131)
        out["mlp6"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), disc.mlp_track_sectors(b), f, 1)
        secs, pcm = raw_pcm(pkg, 711, 0, 40)
        out["pcm6"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), secs, len(pcm), 0)
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=60), 132)
        out["mlp2ss"] = one_track(pkg, tempfile.mkdtemp(dir=tmp), disc.mlp_track_sectors(b), f, 1)
        plain = {}
        for name, ats in out.items():
            plain[name] = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001)
            assert not plain[name]["windowed"] and "downmix" not in plain[name] and plain[name]["channels"] == 6
            assert plain[name]["mask"] == 0x3F == mm.speaker_mask(12)
            plain[name]["pcm"].setflags(write=False)
        yield out, plain


def mixed(plain, och, flags=0):
    """the plain read through the model -> (the mixed track [och, frames], the report)"""
    m = mm.default_matrix(plain["mask"], och, flags)
    want, cl = mm.mix_np(np.ascontiguousarray(plain["pcm"].T), m, plain["bits"])
    return want, mm.report(want.shape[1], cl)


@pytest.mark.parametrize("downmix,och,flags", [(2, 2, 0), (1, 1, 0), ((2, mm.LFE), 2, mm.LFE), ((1, mm.UNITY), 1, mm.UNITY)])
@pytest.mark.parametrize("name,codec", [("mlp6", "MLP"), ("pcm6", "PCM")])
def test_track_mixed(pkg, discs, name, codec, downmix, och, flags):
    """read_track(downmix=) equals the plain read through the model: channels, mask, source channels, report; as PCM and
    as the payload"""
    ats, plain = discs[0][name], discs[1][name]
    rt = pkg.discdec.read_track
    if flags & mm.UNITY:
        # 5.1 to mono at unity gain has a row above 2^31: no matrix the kernels take, no reader
        assert not mm.valid(mm.default_matrix(plain["mask"], och, flags))
        with pytest.raises(RuntimeError, match="cannot be opened"):
            rt(ats, 1, 1, 1, downmix=downmix)
        return
    want, rep = mixed(plain, och, flags)
    got = rt(ats, 1, 1, 1, chunk=3001, downmix=downmix, digest=True, levels=True)
    assert not got["windowed"] and got["codec"] == codec and got["bits"] == plain["bits"] and got["rate"] == plain["rate"]
    assert (got["channels"], got["mask"], got["source_channels"]) == (och, 0x3 if och == 2 else 0x4, 6)
    assert got["downmix_state"] == 1 and got["downmix"] == rep and got["frames"] == plain["frames"]
    assert got["pcm"].shape == (plain["frames"], och) and np.array_equal(got["pcm"].T, want)
    pay = rm.payload(want, 24)
    assert (got["crc32"], got["crc32_bytes"]) == (zlib.crc32(pay), len(pay))
    assert got["levels"]["frames"] == plain["frames"] and got["levels"]["max"][:och] == [int(w.max()) for w in want]
    assert rep["clipped"] == [0] * 8            # NORMALIZED: input inside the depth never clips
    for fused in (False, True):
        packed = rt(ats, 1, 1, 1, wav=True, fused=fused, downmix=downmix)
        assert packed["payload"] == pay and not packed["wav_only"] and packed["channels"] == och
        assert packed["downmix"] == rep


@pytest.mark.parametrize("name", ["mlp6", "pcm6"])
def test_the_stages_behind_the_mix(pkg, discs, name):
    """mix, then decimate or resample, then requantize: the models composed in that order"""
    hd = pkg.hipdec
    ats, plain = discs[0][name], discs[1][name]
    rt = pkg.discdec.read_track
    mix2, rep = mixed(plain, 2)
    if plain["rate"] == 96000:
        low, cl = dm.decimate_np(mix2, hd.decim_taps(2), 2, 24)
        rep_d = dm.report(mix2.shape[1], low.shape[1], cl)
        want, cl = qm.requant_np(low, 24, 16, qm.TPDF, 7, 0)
        got = rt(ats, 1, 1, 1, downmix=2, decimate=2, requant=(16, qm.TPDF, 7), digest=True)
        assert got["decimate"] == rep_d and (got["rate"], got["source_rate"]) == (48000, 96000)
    else:
        low = mix2
    res, cl_r = rm.resample_np(low, hd.resample_taps(), 24)
    want_r, cl_q = qm.requant_np(res, 24, 16, qm.TPDF, 7, 0)
    got_r = rt(ats, 1, 1, 1, downmix=2, resample=44100, requant=(16, qm.TPDF, 7), digest=True)
    assert got_r["resample"] == rm.report(low.shape[1], res.shape[1], cl_r) and got_r["rate"] == 44100
    assert (got_r["resample_decimate"] is None) == (plain["rate"] == 48000)
    if plain["rate"] == 96000:
        assert got_r["resample_decimate"] == rep_d
    else:
        want, cl, got = want_r, cl_q, got_r
    for g, w, c in ((got, want, cl), (got_r, want_r, cl_q)):
        pay = qm.payload(w, 16)
        assert (g["channels"], g["mask"], g["source_channels"], g["bits"], g["source_bits"]) == (2, 0x3, 6, 16, 24)
        assert g["downmix"] == rep and g["requant"] == qm.report(w.shape[1], c)
        assert np.array_equal(g["pcm"].T, w)
        assert (g["crc32"], g["crc32_bytes"]) == (zlib.crc32(pay), len(pay))
    packed = rt(ats, 1, 1, 1, wav=True, fused=True, downmix=2, resample=44100, requant=(16, qm.TPDF, 7))
    assert packed["payload"] == qm.payload(want_r, 16)


def test_a_track_that_has_the_channels_is_untouched(pkg, discs):
    """the 2-channel presentation of a two-substream track: state 0, the track as it is; without the presentation the
    six channels are mixed"""
    ats, plain = discs[0]["mlp2ss"], discs[1]["mlp2ss"]
    rt = pkg.discdec.read_track
    stereo = rt(ats, 1, 1, 1, presentation=1, digest=True)
    assert stereo["channels"] == 2
    got = rt(ats, 1, 1, 1, presentation=1, downmix=2, digest=True)
    assert got["downmix_state"] == 0 and got["downmix"] is None and got["source_channels"] == got["channels"] == 2
    assert got["mask"] == stereo["mask"] and np.array_equal(got["pcm"], stereo["pcm"]) and got["crc32"] == stereo["crc32"]
    for fused in (False, True):
        a, b = (rt(ats, 1, 1, 1, presentation=1, wav=True, fused=fused, **kw) for kw in ({}, dict(downmix=2)))
        assert a["payload"] == b["payload"] and a["wav_only"] == b["wav_only"]
    mono = rt(ats, 1, 1, 1, presentation=1, downmix=1)
    want, cl = mm.mix_np(np.ascontiguousarray(stereo["pcm"].T), mm.default_matrix(stereo["mask"], 1), stereo["bits"])
    assert (mono["channels"], mono["mask"], mono["source_channels"]) == (1, 0x4, 2) and np.array_equal(mono["pcm"].T, want)
    want, rep = mixed(plain, 2)
    got = rt(ats, 1, 1, 1, downmix=2)
    assert got["downmix"] == rep and np.array_equal(got["pcm"].T, want)


def test_refused_opens(pkg, discs):
    """a track the reader would take in windows, conceal mode, channel counts and flags the option does not have: the open
    returns NULL"""
    syn, disc = pkg.synth, pkg.disc
    rt = pkg.discdec.read_track
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=400), 133)
    secs = disc.mlp_track_sectors(b)
    psecs, pcm = raw_pcm(pkg, 714, 0, 80)
    assert len(secs) > 64 and len(psecs) > 64
    with tempfile.TemporaryDirectory() as tmp:
        for s, n, rc in ((secs, f, 1), (psecs, len(pcm), 0)):
            ats = one_track(pkg, tempfile.mkdtemp(dir=tmp), s, n, rc)
            with window_sectors(64):
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
                assert rt(ats, 1, 1, 1)["windowed"]
                with pytest.raises(RuntimeError, match="cannot be opened"):
                    rt(ats, 1, 1, 1, downmix=2)
                pkg.discdec.lib().dvda_hip_release_cached_buffers()
            assert rt(ats, 1, 1, 1, downmix=2)["channels"] == 2
    ats = discs[0]["mlp6"]
    assert rt(ats, 1, 1, 1, downmix=2, conceal=False)["channels"] == 2
    for kw in (dict(downmix=2, conceal=True), dict(downmix=3), dict(downmix=6), dict(downmix=(2, 4)), dict(downmix=(2, 8))):
        with pytest.raises(RuntimeError, match="cannot be opened"):
            rt(ats, 1, 1, 1, **kw)
    # the option is read when a reader is opened and nothing of it is left behind
    L = pkg.discdec.lib()
    d = L.dvda_open(ats.encode(), None)
    ts = L.dvda_open_titleset(d, 1)
    t = L.dvda_open_title(ts, 1)
    k = L.dvda_open_track(t, 1)
    r = L.dvda_open_track_reader(k)
    rep = pkg.hipdec.PcmMixReport(7, (ctypes.c_uint64 * 8)(*[7] * 8))
    assert r and L.dvda_hip_reader_downmixed(r, None) == 0 and L.dvda_hip_reader_downmixed(None, None) == 0
    assert L.dvda_hip_reader_downmixed(r, ctypes.byref(rep)) == 0 and rep.as_dict() == mm.report(7, [7] * 8)
    assert L.dvda_channel_count(r) == L.dvda_hip_reader_source_channels(r) == 6 and L.dvda_hip_reader_source_channels(None) == 0
    assert L.dvda_riff_wave_channel_mask(r) == 0x3F
    L.dvda_close_track_reader(r)
    L.dvda_close_track(k)
    L.dvda_close_title(t)
    L.dvda_close_titleset(ts)
    L.dvda_close(d)


def returned(free_before, slack=16 << 20, seconds=5.0):
    """The device memory of the tool's processes is handed back a moment after they exit, and the reading is
    device-wide: a test behind this file that reads free memory (tests/test_gpu_ownership.py) would see it come back.
    Polls until free memory is what it was before the first of them started -> whether it got there.  This is no
    leak check and its answer is not asserted: the memory is other processes', the reading is shared with whoever else
    uses the device, and what THIS process leaves behind is what tests/test_gpu_ownership.py measures.  When the 5 s
    run out the test goes on as it would without the wait; only the reading of a test behind it is then unprotected."""
    import time
    import torch
    end = time.monotonic() + seconds
    while torch.cuda.mem_get_info(0)[0] + slack < free_before:
        if time.monotonic() > end:
            return False
        time.sleep(0.02)
    return True


def test_tool_downmix_option(pkg, discs):
    """dvda2wav_hip --downmix: the header says 2 channels (mono: 1), the data chunk is the model's payload, one DOWNMIX
    line per track; without the flag the tool writes the six channels as it always did"""
    import torch
    tool = pkg._build.build_tool()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    try:
        tool_cases(pkg, discs, tool)
    finally:
        returned(free_before)


def tool_cases(pkg, discs, tool):
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("mlp6", "pcm6"):
            ats, plain = discs[0][name], discs[1][name]
            for args, och, flags in ((["--downmix"], 2, 0), (["--downmix=mono,lfe"], 1, mm.LFE)):
                want, rep = mixed(plain, och, flags)
                pay = rm.payload(want, 24)
                r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), args)
                assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
                channels, rate, _, align, bits = struct.unpack("<HIIHH", data[22:36])
                assert (channels, rate, align, bits) == (och, plain["rate"], 3 * och, 24)
                assert struct.unpack("<I", data[40:44])[0] == (0x3 if och == 2 else 0x4)
                assert data[68:] == pay
                assert ["DOWNMIX", "1", "1", "1", "6", str(och), str(sum(rep["clipped"]))] in lines
                assert ["CRC32", "1", "1", "1", "%08x" % zlib.crc32(pay), str(len(pay))] in lines
            r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), [])
            assert r.returncode == 0 and not any(ln[:1] == ["DOWNMIX"] for ln in lines)
            channels, rate, _, align, bits = struct.unpack("<HIIHH", data[22:36])
            assert (channels, rate, align, bits) == (6, plain["rate"], 18, 24)
            assert struct.unpack("<I", data[40:44])[0] == 0x3F and data[68:] == rm.payload(plain["pcm"].T, 24)
        # mixed, resampled and reduced in one run: a 16-bit 44.1 kHz stereo file
        ats, plain = discs[0]["pcm6"], discs[1]["pcm6"]
        mix2, _ = mixed(plain, 2)
        res, _ = rm.resample_np(mix2, pkg.hipdec.resample_taps(), 24)
        want, _ = qm.requant_np(res, 24, 16, qm.TPDF, 0, 0)
        r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["--downmix", "-r", "44100", "--resample", "-b", "16"])
        assert r.returncode == 0 and data[68:] == qm.payload(want, 16)
        assert struct.unpack("<HIIHH", data[22:36])[:2] == (2, 44100)
        ats = discs[0]["mlp2ss"]
        r, lines, data = run_tool(tool, ats, tempfile.mkdtemp(dir=tmp), ["--downmix", "--stereo"])
        assert r.returncode == 0 and ["DOWNMIX", "1", "1", "1", "2", "2", "none"] in lines
        for bad in (["--downmix=quad"], ["--downmix", "--conceal"]):
            out = tempfile.mkdtemp(dir=tmp)
            r, _, _ = run_tool(tool, ats, out, bad)
            assert r.returncode != 0 and os.listdir(out) == []
