"""The level report through the disc tier (dvda_hip_set_levels / dvda_hip_reader_levels, discdec.read_track(levels=True)):
a reader's report, made on the device piece by piece and joined as the windows are handed out, is
tests/levels_model.levels of the PCM the same reader delivers.  Every comparison is exact."""
import ctypes
import tempfile

import numpy as np
import pytest

from tests import levels_model as lm
from tests.test_disc_api import _titles
from tests.test_gpu_digest_disc import window_sectors

pytestmark = pytest.mark.gpu


def check_readers(pkg, ats, track, bits, windowed, presentation=0):
    """the int32 reader read with dvda_read() and as payload pieces, and the WAV-payload-only reader, of one track"""
    plain = pkg.discdec.read_track(ats, 1, 1, track, chunk=3001, levels=True, presentation=presentation)
    assert plain["windowed"] == windowed and plain["bits"] == bits and len(plain["pcm"]) > 0
    want = lm.levels(plain["pcm"].T, bits)
    assert plain["levels"] == want
    # not final before a windowed reader is at its end, final after; a whole-track reader: from open on
    assert plain["levels_states"] == ((0, 1) if windowed else (1, 1))
    # the same reader handing out the payload it packs from its int32 PCM: the same report
    w = pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=False, pieces=True, levels=True, presentation=presentation)
    assert w["windowed"] == windowed and not w.get("failed")
    if windowed:
        assert len(w["piece_sizes"]) >= 3           # (the join really happens)
    if windowed or not w["wav_only"]:
        assert w["levels"] == want and w["levels_states"] == ((0, 1) if windowed else (1, 1))
    # a WAV-payload-only reader holds no int32 PCM: no report
    fused = pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=True, pieces=True, levels=True, presentation=presentation)
    if fused["wav_only"]:
        assert fused["levels"] is None and fused["levels_states"] == (-1, -1)
    # beside the digest, and without either
    both = pkg.discdec.read_track(ats, 1, 1, track, chunk=4096, levels=True, digest=True, presentation=presentation)
    assert both["levels"] == want and both["crc32_states"][1] == 1
    assert "levels" not in pkg.discdec.read_track(ats, 1, 1, track, presentation=presentation)
    return plain["pcm"], want


def test_mlp_tracks_long_and_short(pkg, oracle):
    syn, disc = pkg.synth, pkg.disc
    with window_sectors(128):
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=1600), 77)
        secs = disc.mlp_track_sectors(b)
        assert len(secs) > 4 * 128
        with tempfile.TemporaryDirectory() as tmp:
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [len(secs) - 40], [f - 80, 80], 1)])
            a, la = check_readers(pkg, ats, 1, 24, windowed=True)
            z, lz = check_readers(pkg, ats, 2, 24, windowed=False)
            want, r, st = oracle.decode(b, 6, f)
            assert st == 0 and np.array_equal(np.concatenate([a, z]).T, want)
            # the tracks' reports join to the title's
            assert pkg.hipdec.levels_combine(la, lz) == lm.levels(want, 24)


@pytest.mark.parametrize("bps_code,assignment", [(2, 12), (0, 1)])
def test_raw_pcm_tracks_long_and_short(pkg, bps_code, assignment):
    disc = pkg.disc
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    with window_sectors(64):
        n_sec = 400
        per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
        frames = per * n_sec
        pcm = np.random.RandomState(500 + bits).randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(frames, ch))
        pcm[:2 * per + 3] = 0                           # silence over more than a sector at the start
        pcm[frames - 30 * per - 5:] = 0                 # ... and over the whole short track and the long one's end
        secs = disc.pcm_track_sectors(pcm, bps_code, 1, assignment)
        assert len(secs) == n_sec > 4 * 64
        with tempfile.TemporaryDirectory() as tmp:
            cut = n_sec - 24
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [cut], [cut * per, frames - cut * per], 1)])
            a, la = check_readers(pkg, ats, 1, bits, windowed=True)
            z, lz = check_readers(pkg, ats, 2, bits, windowed=False)
            assert np.array_equal(np.concatenate([a, z]), pcm)
            assert la["lead_silent"] == 2 * per + 3 and la["trail_silent"] == 6 * per + 5
            assert lz["lead_silent"] == lz["trail_silent"] == lz["frames"] == 24 * per
            assert pkg.hipdec.levels_combine(la, lz) == lm.levels(pcm.T.astype(np.int32), bits)


def test_presentation(pkg, oracle):
    """the 2-channel presentation of a two-substream track, whole and in windows"""
    syn, disc = pkg.synth, pkg.disc
    with window_sectors(128):
        for n_aus, windowed in ((96, False), (1600, True)):
            b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=n_aus), 78)
            secs = disc.mlp_track_sectors(b)
            with tempfile.TemporaryDirectory() as tmp:
                ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [], [f], 1)])
                pcm, want = check_readers(pkg, ats, 1, 24, windowed=windowed, presentation=1)
                assert pcm.shape == (f, 2) and want["frames"] == f
                assert want["min"][2:] == [0] * 6 and want["over"][2:] == [0] * 6


def test_levels_off_by_default(pkg):
    with tempfile.TemporaryDirectory() as tmp:
        titles, _ = _titles(pkg)
        ats = pkg.disc.write_disc_titles(tmp, titles)
        L = pkg.discdec.lib()
        info = pkg.discdec.read_track(ats, 1, 1, 1)
        assert "levels" not in info
        # (asked of a reader that was opened without it: -1, with or without somewhere to put it)
        d = L.dvda_open(ats.encode(), None)
        ts = L.dvda_open_titleset(d, 1)
        t = L.dvda_open_title(ts, 1)
        k = L.dvda_open_track(t, 1)
        r = L.dvda_open_track_reader(k)
        out = pkg.hipdec.Levels()
        assert r and L.dvda_hip_reader_levels(r, None) == -1 and L.dvda_hip_reader_levels(r, ctypes.byref(out)) == -1
        assert out.as_dict() == lm.zero()
        L.dvda_close_track_reader(r)
        L.dvda_close_track(k)
        L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
        L.dvda_close(d)


def test_option_off_holds_no_more_device_memory(pkg):
    """a windowed reader without the option peaks no higher than one with it: the report's block is the only thing the
    option allocates, and only when it is on.  The peak is read from the device's free memory, which other work on the
    device moves too: the allowance is the one tests/test_disc_api.py gives two reads of the same windows."""
    syn, disc = pkg.synth, pkg.disc
    L = pkg.discdec.lib()
    with window_sectors(128):
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=1600), 77)
        secs = disc.mlp_track_sectors(b)
        with tempfile.TemporaryDirectory() as tmp:
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [], [f], 1)])
            peaks = {}
            for on in (False, True):
                L.dvda_hip_release_cached_buffers()         # (the memory figures: from a clean start)
                info = pkg.discdec.read_track(ats, 1, 1, 1, levels=on)
                assert info["windowed"] and not info["failed"] and ("levels" in info) == on
                peaks[on] = info["device_peak"]
            L.dvda_hip_release_cached_buffers()
            assert 0 < peaks[False] <= 1.35 * peaks[True] + (8 << 20)
