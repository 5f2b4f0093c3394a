"""The track rules of the disc tier at the branches no other test reaches, through both kinds of reader: the look-ahead
behind a track grown once and twice (the next major sync lies more than 8, more than 32 sectors behind it), a window
that holds no cut, a track nothing follows (7 bytes short of the data), the payload the decode writes and its digest
on the same discs, a raw-PCM track that spills over its sector range, and a PTS length of 0.

Every expectation is the CPU oracle's decode of the stream's bytes (raw PCM: the samples that went in).  Every disc is
read with DVDA_WINDOW_SECTORS unset (one batch) and with 64-sector windows (a track of more than 64 sectors is then
windowed and comes in at least 2 pieces; a PTS length of 0 delivers one packet, so one piece)."""
import functools
import os
import tempfile
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOM = 2021                                     # MLP payload bytes a sector carries: byte o lies in sector o // ROOM
MODES = [None, 64]                              # DVDA_WINDOW_SECTORS: unset, 64


class window_sectors:
    """DVDA_WINDOW_SECTORS for the block (None: unset), put back afterwards"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get("DVDA_WINDOW_SECTORS")
        if self.n is None:
            os.environ.pop("DVDA_WINDOW_SECTORS", None)
        else:
            os.environ["DVDA_WINDOW_SECTORS"] = str(self.n)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DVDA_WINDOW_SECTORS", None)
        else:
            os.environ["DVDA_WINDOW_SECTORS"] = self.old


@functools.lru_cache(maxsize=None)
def _stream(restart_interval, n_aus):
    """(bytes, frames, sectors, sectors that hold a major sync, the oracle's PCM [6, frames]) -- made once"""
    import libdvd_audio_amd as pkg
    from tests import oracle_lib
    syn = pkg.synth
    b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, restart_interval=restart_interval,
                                   n_aus=n_aus), 7)
    raw = b.tobytes()
    at, p = [], raw.find(b"\xF8\x72\x6F\xBB")
    while p >= 0:
        at.append((p - 4) // ROOM)              # the unit begins 4 bytes in front of the pattern
        p = raw.find(b"\xF8\x72\x6F\xBB", p + 1)
    want, r, st = oracle_lib.Oracle().decode(b, 6, f)
    assert st == 0 and r == f
    want.setflags(write=False)
    return b, f, pkg.disc.mlp_track_sectors(b), at, want


def _sync_behind(b, cut):
    """sector of the first major sync at or behind the first payload byte of sector `cut`, None when there is none"""
    p = b.tobytes().find(b"\xF8\x72\x6F\xBB", cut * ROOM + 4)
    return None if p < 0 else (p - 4) // ROOM


def _read_both_ways(pkg, oracle, ats, track, n_sectors, window, want):
    """int32 read and payload pieces of one track against `want` [channels, frames]"""
    a = pkg.discdec.read_track(ats, 1, 1, track, chunk=3001)
    windowed = window is not None and n_sectors > window
    assert a["windowed"] == windowed and not a.get("failed")
    assert a["status"] & ~pkg.hipdec.ST_BENIGN == 0 and a["frames"] == len(a["pcm"]) == want.shape[1]
    assert np.array_equal(a["pcm"].T, want)
    w = pkg.discdec.read_track(ats, 1, 1, track, wav=True, pieces=True)
    assert w["windowed"] == windowed and not w.get("failed")
    assert w["payload"] == oracle.wav_pack(want, 24)
    if windowed:
        assert len(w["piece_sizes"]) >= 2


def _two_tracks(pkg, oracle, restart_interval, n_aus, cut, window, window2="same"):
    """a title of two tracks cut at sector `cut`: track 1 is the oracle's decode of the bytes in front of the first
    major sync behind the cut, track 2 the rest of the stream (read at window2 where that is not `window`)"""
    b, f, secs, at, want = _stream(restart_interval, n_aus)
    begin2 = b.tobytes().find(b"\xF8\x72\x6F\xBB", cut * ROOM + 4) - 4
    head, r, st = oracle.decode(b[:begin2], 6, f)
    assert st == 0 and 0 < r < f and np.array_equal(head, want[:, :r])
    with window_sectors(window), tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [cut], [r, f - r], 1)])
        _read_both_ways(pkg, oracle, ats, 1, cut, window, want[:, :r])
    if window2 == "same":
        window2 = window
    with window_sectors(window2), tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [cut], [r, f - r], 1)])
        # track 2 begins at the sync behind the cut: the rest of the stream, and with track 1 all of it
        _read_both_ways(pkg, oracle, ats, 2, len(secs) - cut, window2, want[:, r:])


@pytest.mark.parametrize("window", MODES)
@pytest.mark.parametrize("cut", [60, 120])
def test_look_ahead_grows_once(pkg, oracle, cut, window):
    """restart_interval 64, 512 access units: 236 sectors, syncs in 0, 29, 58, 88, 117, 147, 176, 206.  The first sync at
    or behind sector `cut` lies more than 8 and at most 32 sectors behind the track's last sector: the first look-ahead
    of 8 sectors does not hold it, the second of 32 does.  Track 1 is one batch at 64-sector windows when cut at 60,
    windowed when cut at 120."""
    b, f, secs, at, want = _stream(64, 512)
    assert (len(secs), f) == (236, 40960) and at == [0, 29, 58, 88, 117, 147, 176, 206]
    assert 8 < _sync_behind(b, cut) - (cut - 1) <= 32
    _two_tracks(pkg, oracle, 64, 512, cut, window)


@pytest.mark.parametrize("window", MODES)
def test_look_ahead_grows_twice_and_a_window_holds_no_cut(pkg, oracle, window):
    """restart_interval 160, 800 access units: 367 sectors, syncs in 0, 73, 146, 219, 293.  Cut at 150: the next sync lies
    more than 32 sectors behind the track's last sector (look-aheads of 8, 32, 128), and at 64-sector windows the first
    window holds no sync but the one at byte 0 -- all of it waits for the next window, the carry is more than a window.
    Track 2 is read as one batch both times: its first major sync (sector 219) lies more than a window behind its first
    sector (150), and a windowed reader whose first window holds no major sync does not open -- a known limit of the
    windowed reader, the same before and after the readers were put together from one set of steps."""
    b, f, secs, at, want = _stream(160, 800)
    assert (len(secs), f) == (367, 64000) and at == [0, 73, 146, 219, 293]
    assert _sync_behind(b, 150) - 149 > 32
    assert [s for s in at if s < 64] == [0]
    _two_tracks(pkg, oracle, 160, 800, 150, window, window2=None)


@pytest.mark.parametrize("window", MODES)
def test_nothing_follows_the_track(pkg, oracle, window):
    """The stream of the first case cut at 210, behind the last sync's sector: track 1 has packets behind it but no
    further sync, and ends 7 bytes short of the data (find_major_sync needs 8); track 2 holds no major sync and does
    not open."""
    b, f, secs, at, want = _stream(64, 512)
    assert at[-1] < 210 < len(secs) and _sync_behind(b, 210) is None
    short, r, st = oracle.decode(b[:len(b) - 7], 6, f)
    assert (r, st) == (40880, 0) and np.array_equal(short, want[:, :r])
    with window_sectors(window), tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [210], [r, f - r], 1)])
        _read_both_ways(pkg, oracle, ats, 1, 210, window, short)
        with pytest.raises(RuntimeError):
            pkg.discdec.read_track(ats, 1, 1, 2)


@pytest.mark.parametrize("window", MODES)
@pytest.mark.parametrize("cut", [60, 120])
def test_payload_written_by_the_decode_and_its_digest(pkg, oracle, cut, window):
    """The two discs of the first case, opened for the payload (the decode writes it) with the digest on: the payload is
    the packing of the int32 read, the digest the CRC-32 of that payload."""
    b, f, secs, at, want = _stream(64, 512)
    with window_sectors(window), tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [cut], [f // 2, f - f // 2], 1)])
        got = b""
        for track, n_sectors in ((1, cut), (2, len(secs) - cut)):
            windowed = window is not None and n_sectors > window
            plain = pkg.discdec.read_track(ats, 1, 1, track, chunk=3001)
            payload = oracle.wav_pack(plain["pcm"].T, 24)
            w = pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=True, pieces=True, digest=True)
            assert w["windowed"] == windowed and w["wav_only"] and not w.get("failed")
            assert w["payload"] == payload and len(payload) > 0
            assert (w["crc32"], w["crc32_bytes"]) == (zlib.crc32(payload), len(payload))
            if windowed:
                assert len(w["piece_sizes"]) >= 2
            got += w["payload"]
        assert got == oracle.wav_pack(want, 24)


PER = 110                                       # PCM frames a sector holds: 24 bit, 6 channels


@functools.lru_cache(maxsize=None)
def _pcm():
    import libdvd_audio_amd as pkg
    pcm = np.random.RandomState(7).randint(-(1 << 23), 1 << 23, size=(80 * PER, 6)).astype(np.int32)
    secs = pkg.disc.pcm_track_sectors(pcm, 2, 1, 12)
    assert len(secs) == 80
    pcm.setflags(write=False)
    return pcm, secs


def _read_pcm(pkg, oracle, ats, window, n_sectors, want, pieces):
    a = pkg.discdec.read_track(ats, 1, 1, 1, chunk=3001)
    windowed = window is not None and n_sectors > window
    assert a["codec"] == "PCM" and a["bits"] == 24 and a["channels"] == 6
    assert a["windowed"] == windowed and not a.get("failed")
    assert a["frames"] == len(a["pcm"]) == len(want) and np.array_equal(a["pcm"], want)
    for fused in (False, True):
        w = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=fused, pieces=True)
        assert w["windowed"] == windowed and not w.get("failed")
        assert w["payload"] == oracle.wav_pack(want.T, 24)
        if windowed:
            assert len(w["piece_sizes"]) >= pieces


@pytest.mark.parametrize("window", MODES)
@pytest.mark.parametrize("n_sectors,packets", [(4, 6), (70, 75)])
def test_raw_pcm_track_spills_over_its_sector_range(pkg, oracle, n_sectors, packets, window):
    """80 sectors of random samples; track 1 has the sector range [0, n_sectors) and a PTS length of `packets` sectors'
    frames: one batch reads twice the range and again, the windowed reader (70 sectors at 64) reads on."""
    pcm, secs = _pcm()
    n = packets * PER
    with window_sectors(window), tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [n_sectors], [n, len(pcm) - n], 1)])
        _read_pcm(pkg, oracle, ats, window, n_sectors, pcm[:n], 2)


@pytest.mark.parametrize("window", MODES)
@pytest.mark.parametrize("n_sectors", [4, 70])
def test_raw_pcm_pts_length_zero_delivers_the_opening_packet(pkg, oracle, n_sectors, window):
    pcm, secs = _pcm()
    with window_sectors(window), tempfile.TemporaryDirectory() as tmp:
        ats = pkg.disc.write_disc_titles(tmp, [pkg.disc.split_tracks(secs, [n_sectors], [0, len(pcm)], 1)])
        _read_pcm(pkg, oracle, ats, window, n_sectors, pcm[:PER], 1)
