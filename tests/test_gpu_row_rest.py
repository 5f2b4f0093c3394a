"""The fast pass's row loop outside the slots and the row tail (csrc/mlp_decode.h, docs/history.md A.15): the ring commit
works out the planes of a whole refill turn from one shift of the turn's first dword (ring_turn_off) and no longer keeps
lo_valid; the chunk request takes its test and its granule count from one difference; the wave's cooperative flush hands
the runs' offsets round through one address register, reads the tile through one LDS address and forms a store's
address by a multiply-add.  What that can get wrong is a matter of WHERE in the ring a turn starts and HOW MANY granules
each lane takes in it (the wrap, the mirror plane written by a granule at any of the four places in a turn), of the END of
the buffer (the clamp to the spare bytes with each count), and of WHERE the runs of a wave lie in the PCM buffer -- so
these cases vary exactly those, each bit-exact against the oracle for PCM, frame counts and status, in every layout the
flush serves, into regions in a shuffled order on 16 bytes but on no multiple of 96, guard words round every one of them
and all of them checked.  Every batch is forced onto the lane kernels (lanes_per_segment = 1) and runs with the
cooperative flush forced where it applies (DVDA_COOP_MIN_SEG=1, read when a context is made).

The flush keeps 64-bit store addresses (no scalar base with 32-bit lane offsets was built), so there is no wide-span
fall-back to test: tests/test_gpu_parity.py::test_wave_flush_into_a_pcm_buffer_of_more_than_16_gb covers a wave whose
runs lie either side of element 2^32."""
import numpy as np
import pytest

from tests import test_gpu_ring_refill as R

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
GUARD_WORDS = 64
LAYOUTS = ["interleaved", "planar", "wav24"]


def _layout(hip, layout):
    return {"interleaved": hip.PCM_INTERLEAVED, "planar": hip.PCM_PLANAR, "wav24": hip.PCM_WAV24}[layout]


def _placed(hip, titles, lay, seed):
    """-> (out_off[i], words of the buffer): the titles' regions (hipdec.region_words each) in a seeded shuffled order, each
    on 16 bytes but on no multiple of 96, GUARD_WORDS words between neighbours and at both ends"""
    order = np.random.default_rng(seed).permutation(len(titles))
    out_off, pos = [0] * len(titles), GUARD_WORDS
    for t in order:
        pos = (pos + 3) & ~3
        if pos % 24 == 0:
            pos += 4
        out_off[t] = pos
        pos += hip.region_words(titles[t][1], titles[t][2], lay) + GUARD_WORDS
    assert any(out_off[i] > out_off[i + 1] for i in range(len(titles) - 1))
    assert all(o % 4 == 0 and o % 24 != 0 for o in out_off)
    return out_off, pos


def _check_placed(pkg, oracle, titles, layout, seed, packed=None):
    """decodes the titles (or the packed bytes that hold them) into placed regions of a guard-filled buffer and checks
    status, frame counts, every value or payload byte and every word outside the regions"""
    hip = pkg.hipdec
    lay = _layout(hip, layout)
    n = len(titles)
    rows, chans = [t[1] for t in titles], [t[2] for t in titles]
    out_off, words = _placed(hip, titles, lay, seed)
    batch = hip.Batch([t[0] for t in titles]) if packed is None else hip.Batch(packed=packed)
    ctx = hip.Context(0, n, 1024, R.LANES, lay)
    try:
        ctx.index_batch(batch)
        last = max(o + hip.region_words(r, c, lay) for o, r, c in zip(out_off, rows, chans))
        out = hip.PcmRegions(rows, chans, lay, out_off=out_off, slack=words - last, fill=GUARD)
        assert out.d_pcm.numel() == words
        ctx.decode(*out.ptrs, 0)
        infos = list(ctx.stream_info(n))
        host = out.d_pcm.cpu().numpy()
    finally:
        ctx.close()
    got = hip.cut_regions(host, out_off, rows, chans, [inf.pcm_frames for inf in infos], lay)
    for i, ((b, f, nch, want), g, inf) in enumerate(zip(titles, got, infos)):
        assert inf.status & ~hip.ST_BENIGN == 0, "stream %d status %#x" % (i, inf.status)
        assert inf.pcm_frames == f and inf.channels == nch, (i, inf.pcm_frames, f)
        if layout == "wav24":
            ref = np.frombuffer(oracle.wav_pack(want, 24), np.uint8)
            assert len(g) == len(ref) and np.array_equal(g, ref), "stream %d: first difference at byte %d" % (
                i, int(np.argmax(g != ref)) if len(g) == len(ref) else -1)
        else:
            assert g.shape == want.shape
            assert np.array_equal(g, want), "stream %d differs at %s" % (i, np.argwhere(g != want)[:4].tolist())
    outside = np.ones(len(host), bool)
    for o, r, c in zip(out_off, rows, chans):
        outside[o:o + hip.region_words(r, c, lay)] = False
    assert outside.sum() >= GUARD_WORDS * (n + 1)
    bad = np.flatnonzero(outside & (host.view(np.uint32) != GUARD))
    assert bad.size == 0, "stray stores at words %s" % bad[:8].tolist()
    return infos


# ---------------------------------------------------------------- whole waves, and a wave of two lanes
@pytest.fixture(scope="module")
def recipe_titles(pkg, oracle):
    """65 six-channel 96 kHz recipe titles of 16 access units, two segments each: the first 32 / 64 / 65 of them are
    64 / 128 / 130 segments -- one wave, two waves, two waves and a wave with two live lanes.  A title is some 15 KB
    through a 128-byte ring: every ring position is wrapped over a hundred times, and the lanes of a wave, each at its own
    place in its own stream, start their turns at all eight granule positions of the ring -- so the granule that starts
    the ring, whose first dword goes to the mirror plane too, is the first, second, third or fourth of a turn."""
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=16)
    titles = R._titles(pkg, oracle, [(cfg, 81000 + i) for i in range(65)])
    assert min(len(t[0]) for t in titles) > 100 * 128
    return titles


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_titles", [32, 64, 65], ids=["64_segments", "128_segments", "130_segments"])
def test_whole_waves_and_a_wave_of_two_lanes(pkg, oracle, recipe_titles, n_titles, layout, monkeypatch):
    monkeypatch.setenv("DVDA_COOP_MIN_SEG", "1")
    infos = _check_placed(pkg, oracle, recipe_titles[:n_titles], layout, 21 + n_titles)
    assert all(inf.status == 0 and inf.segments == 2 for inf in infos)


# ---------------------------------------------------------------- lanes of one wave that take 0 .. 4 granules in one turn
@pytest.fixture(scope="module")
def mixed_rate_titles(pkg, oracle):
    """2-channel and 6-channel titles and two huffman_lsbs settings (2 and the generator's largest, 24), title by title:
    the four kinds sit side by side in every wave and eat from under 3 to over 20 bytes a PCM frame, so in the turn
    that the hungriest lane calls the others have room for none, one, two, three or four granules"""
    syn = pkg.synth
    cases = []
    for i in range(66):
        cfg = syn.make_cfg(assignment=12 if i % 2 else 1, rate_code=1, n_substreams=1, n_aus=16,
                           huffman_lsbs=24 if (i // 2) % 2 else 2, restart_interval=8)
        cases.append((cfg, 82000 + i))
    titles = R._titles(pkg, oracle, cases)
    per_frame = [len(b) / f for b, f, _, _ in titles]
    kinds = [per_frame[k::4] for k in range(4)]         # 2ch/2, 6ch/2, 2ch/24, 6ch/24
    assert max(kinds[0]) < 3.0 and min(kinds[3]) >= 20.0, (max(kinds[0]), min(kinds[3]))
    assert max(kinds[0]) < min(kinds[1]) and max(kinds[1]) < min(kinds[3]) and max(kinds[0]) < min(kinds[2])
    return titles


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mixed_rates_in_one_wave(pkg, oracle, mixed_rate_titles, layout, monkeypatch):
    monkeypatch.setenv("DVDA_COOP_MIN_SEG", "1")
    _check_placed(pkg, oracle, mixed_rate_titles, layout, 5)


# ---------------------------------------------------------------- the clamp to the spare bytes
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("within", [64, 48, 32, 16])
def test_last_access_unit_ends_near_the_end_of_the_buffer(pkg, oracle, recipe_titles, within, layout, monkeypatch):
    """The batch's last title ends inside the last `within` bytes of the batch buffer (and not inside the last
    `within` - 16), zeros behind it, then only the 64 spare bytes: the last turns of the lanes that read the buffer's end ask
    for granules past it, one to four of them, and take them from the buffer's last granules instead"""
    monkeypatch.setenv("DVDA_COOP_MIN_SEG", "1")
    hip = pkg.hipdec
    titles = list(recipe_titles[:34])                       # 68 segments: a whole wave and four lanes
    k = next(i for i in range(len(titles) - 1, -1, -1) if len(titles[i][0]) % 16 != 0)
    titles = titles[:k] + titles[k + 1:] + [titles[k]]
    flat, offs, lens = hip.pack_streams([t[0] for t in titles])
    flat = np.concatenate([flat[:-64], np.zeros(within - 16, np.uint8), flat[-64:]])
    total, end = len(flat) - 64, int(offs[-1] + lens[-1])
    assert within - 16 < total - end < within and total % 16 == 0
    _check_placed(pkg, oracle, titles, layout, 40 + within, packed=(flat, offs, lens))
