"""The host arithmetic of hipdec's output side (region_layout, cut_regions, grown_rows, standard_rows): needs no GPU."""
import numpy as np
import pytest

ROWS, CHANNELS = [80, 0, 41], [6, 2, 5]


def _layouts(hd):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24, "wav16": hd.PCM_WAV16}


@pytest.mark.parametrize("layout,offsets,words", [("planar", [0, 480, 480], 685), ("interleaved", [0, 480, 480], 685),
                                                   ("wav24", [0, 364, 368], 526), ("wav16", [0, 244, 248], 355)])
def test_region_layout_table(pkg, layout, offsets, words):
    """r*c words for the int32 layouts, (r*c*nb + 3)//4 + 4 for the WAV ones: the values worked out by hand"""
    hd = pkg.hipdec
    assert hd.region_layout(ROWS, CHANNELS, _layouts(hd)[layout]) == (offsets, words)


def test_a_buffer_is_never_shorter_than_one_word(pkg):
    hd = pkg.hipdec
    for lay in (hd.PCM_PLANAR, hd.PCM_INTERLEAVED):
        assert hd.region_layout([0, 0, 0], CHANNELS, lay) == ([0, 0, 0], 1)     # all rows 0
    assert hd.region_layout([], [], hd.PCM_WAV24) == ([], 1)


@pytest.mark.parametrize("layout", ["planar", "interleaved", "wav24", "wav16"])
def test_cutting(pkg, layout):
    """a buffer written the way the kernels write it comes back as exactly the contents, cut to pcm_frames; a zero-row
    stream is [c, 0]; pcm_frames above rows is cut at rows"""
    hd = pkg.hipdec
    lay = _layouts(hd)[layout]
    nb = hd.sample_bytes(lay)
    rng = np.random.default_rng(7)
    frames = [60, 5, 50]                        # below rows; above rows == 0; above rows
    out_off, words = hd.region_layout(ROWS, CHANNELS, lay)
    host = np.full(words, 0x5A5A5A5A, np.int32)
    want = []
    for o, r, c in zip(out_off, ROWS, CHANNELS):
        if nb == 4:
            p = rng.integers(-2 ** 31, 2 ** 31, (c, r), dtype=np.int64).astype(np.int32)
            host[o:o + r * c] = (p.T if layout == "interleaved" else p).reshape(-1)
        else:
            p = rng.integers(0, 256, r * c * nb, dtype=np.int64).astype(np.uint8)
            host.view(np.uint8)[4 * o:4 * o + r * c * nb] = p
        want.append(p)
    got = hd.cut_regions(host, out_off, ROWS, CHANNELS, frames, lay)
    for g, w, r, c, f in zip(got, want, ROWS, CHANNELS, frames):
        f = min(f, r)
        if nb == 4:
            assert g.dtype == np.int32 and g.shape == (c, f) and np.array_equal(g, w[:, :f])
        else:
            assert g.dtype == np.uint8 and g.shape == (f * c * nb,) and np.array_equal(g, w[:f * c * nb])
    if nb == 4:
        assert got[1].shape == (2, 0)


def test_growing_and_standard_rows(pkg):
    hd = pkg.hipdec
    infos = (hd.StreamInfo * 4)()
    for inf, (aus, rate, frames) in zip(infos, [(10, 1, 800), (10, 0, 401), (3, 2, 0), (7, 5, 9)]):
        inf.mlp_frames, inf.group0_rate, inf.pcm_frames = aus, rate, frames
    rows = [hd.standard_rows(inf) for inf in infos]
    assert rows == [800, 400, 480, 0]           # 80 / 40 / 160 rows per access unit; a rate the table does not know: 0
    assert hd.grown_rows(rows, infos) == [800, 401, 480, 9]     # changed only where a stream asks for more
    assert rows == [800, 400, 480, 0]
