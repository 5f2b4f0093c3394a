"""The PCM digest and the level report side by side (csrc/pcm_report_run.h, csrc/disc_reader.c piece_reports): on a context
they share one descriptor array, one result block and one workspace, and the disc tier makes both of a piece in one block
on the device -- so each must come out as it does alone, whatever the other left behind.  The same holds of all seven
passes behind a decode, which share one staging path (report_of_decode).  Every comparison is exact."""
import ctypes
import tempfile
import zlib

import numpy as np
import pytest

from tests import compare_model as cm
from tests import decimate_model as dm
from tests import digest_model as dgm
from tests import energy_model as em
from tests import levels_model as lm
from tests import requant_model as rm
from tests import resample_model as rsm
from tests.test_disc_api import _titles
from tests.test_gpu_digest_disc import window_sectors

pytestmark = pytest.mark.gpu

AU = 80                 # PCM frames per access unit at 96 kHz


def _decode(hd, ctx, streams, layout):
    """index + decode of `streams` on ctx -> (regions, the stream handle, PCM on the host as [channels, frames])"""
    batch = hd.Batch(streams)
    st = batch.current_stream
    ctx.index_batch(batch, st)
    out = hd.PcmRegions.for_infos(ctx.stream_info(stream=st), layout)
    ctx.decode(*out.ptrs, st)
    infos = ctx.stream_info(stream=st)
    assert not any(inf.status & ~hd.ST_BENIGN for inf in infos)
    return out, st, out.to_host(infos)


def _digests(oracle, pcm, bits):
    payloads = [oracle.wav_pack(p, bits) for p in pcm]
    return [(zlib.crc32(p), len(p)) for p in payloads]


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_interleaved_on_one_context(pkg, oracle, layout):
    hd, syn = pkg.hipdec, pkg.synth
    lay = {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED}[layout]
    # one ragged tile of each kind | two level tiles, two digest tiles at 24 bits | two level tiles, six digest tiles
    shapes = [(1, 1), (1, 60), (12, 60)]
    streams = [syn.stream(syn.make_cfg(assignment=a, rate_code=1, n_substreams=1, n_aus=n), 40 + i)
               for i, (a, n) in enumerate(shapes)]
    assert [f for _, f in streams] == [AU, 60 * AU, 60 * AU]
    assert 60 * AU > lm.TILE and 16384 < 60 * AU * 2 * 3 <= 2 * 16384 and 5 * 16384 < 60 * AU * 6 * 3 <= 6 * 16384
    ctx = hd.Context(0, 3, 4096, 0, lay)
    try:
        out, st, pcm = _decode(hd, ctx, [b for b, _ in streams], lay)
        assert [p.shape for p in pcm] == [(2, AU), (2, 60 * AU), (6, 60 * AU)]
        levels = {bits: [lm.levels(p, bits) for p in pcm] for bits in (16, 24)}
        digests = {bits: _digests(oracle, pcm, bits) for bits in (16, 24)}
        assert ctx.pcm_levels(*out.ptrs, 24, stream=st) == levels[24]
        assert ctx.pcm_crc32(*out.ptrs, 24, stream=st) == digests[24]
        assert ctx.pcm_levels(*out.ptrs, 16, stream=st) == levels[16]
        assert ctx.pcm_crc32(*out.ptrs, 16, stream=st) == digests[16]
        assert ctx.pcm_levels(*out.ptrs, 24, stream=st) == levels[24]
        # a short batch behind it: nothing grows, and the workspace is full of the first batch's records
        short, f = syn.stream(syn.make_cfg(assignment=1, rate_code=1, n_substreams=1, n_aus=3), 50)
        out, st, pcm = _decode(hd, ctx, [short], lay)
        assert [p.shape for p in pcm] == [(2, f)] and f == 3 * AU
        assert ctx.pcm_crc32(*out.ptrs, 24, stream=st) == _digests(oracle, pcm, 24)
        assert ctx.pcm_levels(*out.ptrs, 24, stream=st) == [lm.levels(pcm[0], 24)]
    finally:
        ctx.close()


def _seven_passes(hd, ctx, out, st, pcm, infos):
    """Every Context.pcm_* call on one decoded batch, interleaved: energy (B = 64), digest 24, decimate by 2 into a second
    tensor, resample into a third, levels 24, compare against a clone with one value changed, requantize 24 -> 16 in
    place, resample again, digest 16, levels 16, energy -- each exactly its model's of the host copy of the PCM as it was
    at that point"""
    import torch
    lay, n = out.layout, len(pcm)
    table = hd.resample_taps()

    def resample(now, bits):
        """(the resampler stages output descriptors of its own behind the caller's, as the decimator does)"""
        desc_rs, words = hd.resample_desc_out(desc)
        d_rs = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=out.dev)
        want = [rsm.resample_np(p, table, bits) for p in now]
        assert ctx.pcm_resample(*out.ptrs, bits, d_rs.data_ptr(), lay, [d[0] for d in desc_rs], [d[1] for d in desc_rs],
                                stream=st) == [rsm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(now, want)]
        got = hd.cut_regions(d_rs.cpu().numpy(), *[[d[k] for d in desc_rs] for k in (0, 1)], out.channels,
                             [d[2] for d in desc_rs], lay)
        assert all(np.array_equal(g, w) for g, (w, _) in zip(got, want))

    def energy(now):
        assert ctx.pcm_energy(*out.ptrs, 64, stream=st) == [em.energy_fast(p, 64) for p in now]

    def digest(now, bits):
        want = [(zlib.crc32(dgm.wav_payload(p, bits)), p.size * (bits // 8)) for p in now]
        assert ctx.pcm_crc32(*out.ptrs, bits, stream=st) == want

    energy(pcm)
    digest(pcm, 24)
    desc = [(o, r, p.shape[1], c) for o, r, p, c in zip(out.out_off, out.rows, pcm, out.channels)]
    desc_low, words = hd.decim_desc_out(desc, 2)
    d_low = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=out.dev)
    low = [dm.decimate_np(p, hd.decim_taps(2), 2, 24) for p in pcm]
    assert ctx.pcm_decimate(*out.ptrs, 2, 24, d_low.data_ptr(), lay, [d[0] for d in desc_low], [d[1] for d in desc_low],
                            stream=st) == [dm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(pcm, low)]
    got = hd.cut_regions(d_low.cpu().numpy(), *[[d[k] for d in desc_low] for k in (0, 1)], out.channels,
                         [d[2] for d in desc_low], lay)
    assert all(np.array_equal(g, w) for g, (w, _) in zip(got, low))
    resample(pcm, 24)
    assert ctx.pcm_levels(*out.ptrs, 24, stream=st) == [lm.levels(p, 24) for p in pcm]
    # side B: the decode's buffer with the last stream's value at (channel 1, frame 70) one higher
    other, c, f = [p.copy() for p in pcm], 1, 70
    other[-1][c, f] += 1
    d_other = out.d_pcm.clone()
    d_other[out.out_off[-1] + (f * out.channels[-1] + c if lay == hd.PCM_INTERLEAVED else c * out.rows[-1] + f)] += 1
    diffs = ctx.pcm_compare(*out.ptrs, d_other, lay, desc, 0, stream=st)
    assert diffs == [cm.diff(a, b, 0) for a, b in zip(pcm, other)] and [d["diff_frames"] for d in diffs] == [0] * (n - 1) + [1]
    frame0 = [3, 0, 2 ** 40 - 5][:n]
    want = [rm.requant_np(p, 24, 16, rm.TPDF, 77, f0) for p, f0 in zip(pcm, frame0)]
    assert ctx.pcm_requantize(*out.ptrs, 24, 16, hd.RQ_TPDF, seed=77, frame0=frame0, stream=st) == \
        [rm.report(p.shape[1], cl) for p, (_, cl) in zip(pcm, want)]
    pcm16 = out.to_host(infos)
    assert all(np.array_equal(a, w) for a, (w, _) in zip(pcm16, want))
    resample(pcm16, 16)
    digest(pcm16, 16)
    assert ctx.pcm_levels(*out.ptrs, 16, stream=st) == [lm.levels(p, 16) for p in pcm16]
    energy(pcm16)


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_all_seven_passes_on_one_context(pkg, layout):
    """the seven passes share one staging path and one result block with seven different layouts: each comes out as it
    does alone, and a one-stream batch behind the longer one shows nothing stale"""
    hd, syn = pkg.hipdec, pkg.synth
    lay = {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED}[layout]
    streams = [syn.stream(syn.make_cfg(assignment=a, rate_code=1, n_substreams=1, n_aus=n), 40 + i)[0]
               for i, (a, n) in enumerate([(1, 1), (1, 60), (12, 60)])]
    short = syn.stream(syn.make_cfg(assignment=1, rate_code=1, n_substreams=1, n_aus=3), 50)[0]
    ctx = hd.Context(0, 3, 4096, 0, lay)
    try:
        for batch, shapes in ((streams, [(2, AU), (2, 60 * AU), (6, 60 * AU)]), ([short], [(2, 3 * AU)])):
            out, st, pcm = _decode(hd, ctx, batch, lay)
            assert [p.shape for p in pcm] == shapes
            _seven_passes(hd, ctx, out, st, pcm, ctx.stream_info(stream=st))
    finally:
        ctx.close()


def check_both_options(pkg, ats, track, windowed):
    """a reader with both options reports what a reader with each option alone reports, and delivers the same PCM"""
    rd = pkg.discdec.read_track
    both = rd(ats, 1, 1, track, chunk=3001, digest=True, levels=True)
    dg = rd(ats, 1, 1, track, chunk=3001, digest=True)
    lv = rd(ats, 1, 1, track, chunk=3001, levels=True)
    assert both["windowed"] == dg["windowed"] == lv["windowed"] == windowed and len(both["pcm"]) > 0
    assert np.array_equal(both["pcm"], dg["pcm"]) and np.array_equal(both["pcm"], lv["pcm"])
    for key in ("crc32", "crc32_bytes", "crc32_states"):
        assert both[key] == dg[key], key
    for key in ("levels", "levels_states"):
        assert both[key] == lv[key], key
    assert both["crc32_states"] == both["levels_states"] == ((0, 1) if windowed else (1, 1))
    assert both["crc32"] is not None and both["levels"]["frames"] == len(both["pcm"])
    # a WAV-payload-only reader: no level report, and the digest it has alone
    fused = rd(ats, 1, 1, track, wav=True, fused=True, pieces=True, digest=True, levels=True)
    if fused["wav_only"]:
        alone = rd(ats, 1, 1, track, wav=True, fused=True, pieces=True, digest=True)
        assert fused["levels"] is None and fused["levels_states"] == (-1, -1)
        for key in ("crc32", "crc32_bytes", "crc32_states"):
            assert fused[key] == alone[key] and fused[key] == dg[key], key
    return fused["wav_only"]


def test_mlp_tracks_both_options(pkg):
    syn, disc = pkg.synth, pkg.disc
    with window_sectors(128):
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=1600), 77)
        secs = disc.mlp_track_sectors(b)
        assert len(secs) > 4 * 128
        with tempfile.TemporaryDirectory() as tmp:
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [len(secs) - 40], [f - 80, 80], 1)])
            wav_only = [check_both_options(pkg, ats, 1, windowed=True), check_both_options(pkg, ats, 2, windowed=False)]
            assert any(wav_only)                    # (the WAV-payload rule was really asked)


def test_raw_pcm_tracks_both_options(pkg):
    disc = pkg.disc
    bps_code, assignment = 2, 12
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    assert (ch, bits) == (6, 24)
    with window_sectors(64):
        n_sec = 400
        per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
        frames = per * n_sec
        pcm = np.random.RandomState(500 + bits).randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(frames, ch))
        pcm[:2 * per + 3] = 0
        pcm[frames - 30 * per - 5:] = 0
        secs = disc.pcm_track_sectors(pcm, bps_code, 1, assignment)
        assert len(secs) == n_sec > 4 * 64
        with tempfile.TemporaryDirectory() as tmp:
            cut = n_sec - 24
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [cut], [cut * per, frames - cut * per], 1)])
            check_both_options(pkg, ats, 1, windowed=True)
            check_both_options(pkg, ats, 2, windowed=False)


def test_neither_option(pkg):
    """a reader opened with neither option: both getters answer -1"""
    with tempfile.TemporaryDirectory() as tmp:
        titles, _ = _titles(pkg)
        ats = pkg.disc.write_disc_titles(tmp, titles)
        L = pkg.discdec.lib()
        d = L.dvda_open(ats.encode(), None)
        ts = L.dvda_open_titleset(d, 1)
        t = L.dvda_open_title(ts, 1)
        k = L.dvda_open_track(t, 1)
        r = L.dvda_open_track_reader(k)
        crc, nbytes, out = ctypes.c_uint(), ctypes.c_ulonglong(), pkg.hipdec.Levels()
        assert r and L.dvda_hip_reader_crc32(r, ctypes.byref(crc), ctypes.byref(nbytes)) == -1 and \
            L.dvda_hip_reader_levels(r, ctypes.byref(out)) == -1
        assert (crc.value, nbytes.value) == (0, 0) and out.as_dict() == lm.zero()
        L.dvda_close_track_reader(r)
        L.dvda_close_track(k)
        L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
        L.dvda_close(d)
