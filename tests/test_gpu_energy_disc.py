"""The energy report through the disc tier (dvda_hip_set_energy / dvda_hip_reader_energy, discdec.read_track(energy=B)):
a reader's blocks, made on the device piece by piece on the track's grid and joined as the windows are handed out, are
tests/energy_model of the PCM the same reader delivers -- whole-track and windowed alike.  Every comparison is exact."""
import ctypes
import tempfile

import numpy as np
import pytest

from tests import energy_model as em
from tests.test_conceal_disc_model import DAMAGES, KINDS, model_of
from tests.test_disc_api import _titles
from tests.test_gpu_digest_disc import window_sectors

pytestmark = pytest.mark.gpu


def read_both(pkg, ats, B, window, **kw):
    """the track as one batch and in windows of `window` sectors -> the whole-track read (the two are compared here)"""
    whole = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001, energy=B, **kw)
    assert not whole["windowed"] and len(whole["pcm"]) > 0
    want = em.energy_fast(whole["pcm"].T, B)
    assert whole["energy"] == want and whole["energy_states"] == (1, 1)
    assert whole["energy_counts"] == (len(want), len(want))
    with window_sectors(window):
        pkg.discdec.lib().dvda_hip_release_cached_buffers()
        win = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001, energy=B, **kw)
        assert win["windowed"] and not win.get("failed") and np.array_equal(win["pcm"], whole["pcm"])
        assert win["energy"] == want
        # not final, and not all there, before the track has been read to its end
        assert win["energy_states"] == (0, 1) and win["energy_counts"][0] < win["energy_counts"][1] == len(want)
        # the same reader handing out the payload it packs from its int32 PCM: the same blocks
        packed = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=False, pieces=True, energy=B, **kw)
        assert packed["windowed"] and len(packed["piece_sizes"]) >= 3 and packed["energy"] == want
        # a WAV-payload-only reader holds no int32 PCM: no report
        fused = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=True, pieces=True, energy=B, **kw)
        if fused["wav_only"]:
            assert fused["energy"] is None and fused["energy_states"] == (-1, -1)
        pkg.discdec.lib().dvda_hip_release_cached_buffers()
    return whole, want


def test_mlp_track(pkg, oracle):
    syn, disc = pkg.synth, pkg.disc
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=1600), 77)
    secs = disc.mlp_track_sectors(b)
    assert len(secs) > 4 * 128
    pcm, r, st = oracle.decode(b, 6, f)
    assert st == 0 and r == f
    with tempfile.TemporaryDirectory() as tmp:
        ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [], [f], 1)])
        for B in (64, 9600):                        # 9600: a tenth of the track's sample rate
            whole, want = read_both(pkg, ats, B, 128)
            assert whole["rate"] == 96000 and np.array_equal(whole["pcm"].T, pcm) and want == em.energy_fast(pcm, B)
        # beside the other reports; and with the option off they are what they are without it
        both = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, levels=True, energy=9600)
        plain = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, levels=True)
        assert both["energy"] == want and "energy" not in plain
        assert (both["crc32"], both["crc32_bytes"], both["levels"]) == (plain["crc32"], plain["crc32_bytes"], plain["levels"])
        with window_sectors(128):
            win = pkg.discdec.read_track(ats, 1, 1, 1, digest=True, levels=True)
            assert win["windowed"] and (win["crc32"], win["levels"]) == (plain["crc32"], plain["levels"])
            pkg.discdec.lib().dvda_hip_release_cached_buffers()
        # a block length the report does not take: the reader has none
        bad = pkg.discdec.read_track(ats, 1, 1, 1, energy=63)
        assert bad["energy"] is None and bad["energy_states"] == (-1, -1)


def test_raw_pcm_track(pkg):
    disc = pkg.disc
    bps_code, assignment = 2, 12
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    n_sec = 400
    per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
    frames = per * n_sec
    pcm = np.random.RandomState(501).randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(frames, ch))
    secs = disc.pcm_track_sectors(pcm, bps_code, 1, assignment)
    assert len(secs) == n_sec > 4 * 64
    with tempfile.TemporaryDirectory() as tmp:
        ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [], [frames], 1)])
        for B in (64, 9600):
            whole, want = read_both(pkg, ats, B, 64)
            assert np.array_equal(whole["pcm"], pcm) and len(want) == em.nblocks(frames, B)


def test_damaged_track_in_conceal_mode(pkg, oracle):
    """the composed track -- kept PCM, silence, PCM of a fresh decoder -- on one grid: the silent windows are pieces too"""
    S, feat = KINDS[0]
    sectors, D, want_pcm, want_spans = model_of(pkg, oracle, S, feat, sorted(DAMAGES)[0])
    assert want_spans and len(sectors) > 4 * 64
    with tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(sectors, [], [want_pcm.shape[1]], 1)])
        whole, want = read_both(pkg, ats, 4800, 64, conceal=True)
        assert np.array_equal(whole["pcm"].T, want_pcm) and whole["status"] & pkg.hipdec.ST_CONCEALED
        first, n = whole["concealed"][0][0], whole["concealed"][0][1]
        silent = [j for j in range(len(want)) if 4800 * j >= first and 4800 * (j + 1) <= first + n]
        assert all(want[j]["peak"] == [0] * 8 for j in silent)


def test_energy_off_by_default(pkg):
    with tempfile.TemporaryDirectory() as tmp:
        titles, _ = _titles(pkg)
        ats = pkg.disc.write_disc_titles(tmp, titles)
        L = pkg.discdec.lib()
        assert "energy" not in pkg.discdec.read_track(ats, 1, 1, 1)
        # (asked of a reader that was opened without it: -1, and nothing is written)
        d = L.dvda_open(ats.encode(), None)
        ts = L.dvda_open_titleset(d, 1)
        t = L.dvda_open_title(ts, 1)
        k = L.dvda_open_track(t, 1)
        r = L.dvda_open_track_reader(k)
        arr = (pkg.hipdec.EnergyBlock * 2)()
        n = ctypes.c_ulonglong(77)
        assert r and L.dvda_hip_reader_energy(r, None, 0, None) == -1
        assert L.dvda_hip_reader_energy(r, arr, 2, ctypes.byref(n)) == -1 and n.value == 77 and bytes(arr) == bytes(336)
        L.dvda_close_track_reader(r)
        L.dvda_close_track(k)
        L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
        L.dvda_close(d)
