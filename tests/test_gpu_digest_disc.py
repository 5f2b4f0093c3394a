"""The PCM digest through the disc tier (dvda_hip_set_digest / dvda_hip_reader_crc32, discdec.read_track(digest=True),
dvda2wav_hip --crc): a reader's CRC-32, computed on the device piece by piece and joined as the windows are handed
out, is zlib.crc32 of the payload the same reader delivers.  Every comparison is exact."""
import os
import re
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from tests.test_disc_api import _titles

pytestmark = pytest.mark.gpu


class window_sectors:
    """DVDA_WINDOW_SECTORS for the block, put back afterwards"""

    def __init__(self, n):
        self.n = str(n)

    def __enter__(self):
        self.old = os.environ.get("DVDA_WINDOW_SECTORS")
        os.environ["DVDA_WINDOW_SECTORS"] = self.n

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["DVDA_WINDOW_SECTORS"]
        else:
            os.environ["DVDA_WINDOW_SECTORS"] = self.old


def check_readers(pkg, oracle, ats, track, bits, windowed):
    """int32, packed and fused readers of one track: the digest is the CRC of what each of them delivered"""
    plain = pkg.discdec.read_track(ats, 1, 1, track, chunk=3001, digest=True)
    payload = oracle.wav_pack(plain["pcm"].T, bits)
    assert plain["windowed"] == windowed and len(payload) > 0
    assert (plain["crc32"], plain["crc32_bytes"]) == (zlib.crc32(payload), len(payload))
    for fused in (False, True):
        w = pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=fused, pieces=True, digest=True)
        assert w["windowed"] == windowed and not w.get("failed") and w["payload"] == payload
        if windowed:
            assert len(w["piece_sizes"]) >= 4           # (the join really happens)
        assert (w["crc32"], w["crc32_bytes"]) == (zlib.crc32(w["payload"]), len(w["payload"]))
        # not final before a windowed reader is at its end, final after; a whole-track reader: from open on
        assert w["crc32_states"] == ((0, 1) if windowed else (1, 1))
    assert plain["crc32_states"] == ((0, 1) if windowed else (1, 1))
    # the one-piece interface of the same reader, and a reader without the digest
    whole = pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=True, digest=True)
    assert (whole["crc32"], whole["crc32_bytes"]) == (zlib.crc32(payload), len(payload))
    assert "crc32" not in pkg.discdec.read_track(ats, 1, 1, track, wav=True, fused=True)
    return payload


def test_mlp_tracks_long_and_short(pkg, oracle):
    syn, disc = pkg.synth, pkg.disc
    with window_sectors(128):
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=1600), 77)
        secs = disc.mlp_track_sectors(b)
        assert len(secs) > 4 * 128
        with tempfile.TemporaryDirectory() as tmp:
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [len(secs) - 40], [f - 80, 80], 1)])
            a = check_readers(pkg, oracle, ats, 1, 24, windowed=True)
            z = check_readers(pkg, oracle, ats, 2, 24, windowed=False)
            want, r, st = oracle.decode(b, 6, f)
            assert st == 0 and a + z == oracle.wav_pack(want, 24)
            # the tracks' digests join to the title's
            ca, cz = zlib.crc32(a), zlib.crc32(z)
            assert pkg.hipdec.crc32_combine(ca, cz, len(z)) == zlib.crc32(a + z)


@pytest.mark.parametrize("bps_code,assignment", [(2, 12), (0, 1)])
def test_raw_pcm_tracks_long_and_short(pkg, oracle, bps_code, assignment):
    disc = pkg.disc
    ch, bits = disc.CHANNELS[assignment], disc.BPS[bps_code]
    with window_sectors(64):
        n_sec = 400
        per = (2048 - 14 - 6 - 7 - 9) // (2 * ch * (bits // 8)) * 2
        frames = per * n_sec
        pcm = np.random.RandomState(500 + bits).randint(-(1 << (bits - 1)), 1 << (bits - 1), size=(frames, ch))
        secs = disc.pcm_track_sectors(pcm, bps_code, 1, assignment)
        assert len(secs) == n_sec > 4 * 64
        with tempfile.TemporaryDirectory() as tmp:
            cut = n_sec - 24
            ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [cut], [cut * per, frames - cut * per], 1)])
            a = check_readers(pkg, oracle, ats, 1, bits, windowed=True)
            z = check_readers(pkg, oracle, ats, 2, bits, windowed=False)
            assert a + z == oracle.wav_pack(pcm.astype(np.int32).T, bits)


def test_presentation(pkg, oracle):
    """--stereo's reader: the 2-channel presentation of a two-substream track, whole and in windows"""
    syn, disc = pkg.synth, pkg.disc
    with window_sectors(128):
        for n_aus, windowed in ((96, False), (1600, True)):
            b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=n_aus), 78)
            secs = disc.mlp_track_sectors(b)
            with tempfile.TemporaryDirectory() as tmp:
                ats = disc.write_disc_titles(tmp, [disc.split_tracks(secs, [], [f], 1)])
                for fused in (False, True):
                    w = pkg.discdec.read_track(ats, 1, 1, 1, wav=True, fused=fused, pieces=True, presentation=1, digest=True)
                    assert w["channels"] == 2 and w["windowed"] == windowed
                    assert len(w["payload"]) == f * 2 * 3
                    assert (w["crc32"], w["crc32_bytes"]) == (zlib.crc32(w["payload"]), len(w["payload"]))


def test_digest_off_by_default(pkg):
    with tempfile.TemporaryDirectory() as tmp:
        titles, _ = _titles(pkg)
        ats = pkg.disc.write_disc_titles(tmp, titles)
        L = pkg.discdec.lib()
        info = pkg.discdec.read_track(ats, 1, 1, 1)
        assert "crc32" not in info
        # (asked of a reader that was opened without it: -1)
        d = L.dvda_open(ats.encode(), None)
        ts = L.dvda_open_titleset(d, 1)
        t = L.dvda_open_title(ts, 1)
        k = L.dvda_open_track(t, 1)
        r = L.dvda_open_track_reader(k)
        assert r and L.dvda_hip_reader_crc32(r, None, None) == -1
        L.dvda_close_track_reader(r)
        L.dvda_close_track(k)
        L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
        L.dvda_close(d)


@pytest.mark.parametrize("extra", [[], ["--stereo"], ["--devices", "0,0"]])
def test_extractor_prints_the_crc_of_what_it_wrote(pkg, extra):
    """build/dvda2wav_hip --crc: one line per track, CRC32 <titleset> <title> <track> <crc> <bytes>, of the data chunk
    of the file it wrote (a long MLP track read in windows among them)"""
    syn, disc = pkg.synth, pkg.disc
    tool = pkg._build.build_tool()
    with window_sectors(128), tempfile.TemporaryDirectory() as tmp:
        titles, _ = _titles(pkg)
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=1600), 79)
        titles.append(disc.split_tracks(disc.mlp_track_sectors(b), [], [f], 1))
        pcm = np.random.RandomState(3).randint(-32768, 32768, size=(3000, 2))
        titles.append(disc.split_tracks(disc.pcm_track_sectors(pcm, 0, 0, 1), [2, 4], [1004, 1004, 992], 0))
        ats = disc.write_disc_titles(tmp, titles)
        out = os.path.join(tmp, "out")
        os.makedirs(out)
        r = subprocess.run([tool, "-A", ats, "-d", out, "--crc"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = {}
        for m in re.finditer(r"^CRC32 (\d+) (\d+) (\d+) ([0-9a-f]{8}) (\d+)$", r.stdout, re.M):
            lines[(int(m.group(2)), int(m.group(3)))] = (int(m.group(1)), int(m.group(4), 16), int(m.group(5)))
        files = sorted(os.listdir(out))
        assert len(files) == len(lines) == 9
        for name in files:
            ti, ki = map(int, re.match(r"track-(\d+)-(\d+)\.wav$", name).groups())
            data = open(os.path.join(out, name), "rb").read()[68:]          # (the tool's header: 68 bytes)
            assert lines[(ti, ki)] == (1, zlib.crc32(data), len(data)), name
