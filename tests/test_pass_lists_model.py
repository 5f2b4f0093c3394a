"""The premises of tests/pass_list_cases.py, from the models under tests/*_model.py and the constants of the headers alone
(no GPU): that every case of tests/test_gpu_pass_lists.py reaches the place of the tile-list driver or of a kernel it is
there for -- the chunk sizes and partial chunks of parts A, the turns, the scan's form and the cut of part B, the join's
second turn of part C, the full count fields of part D."""
import numpy as np
import pytest

from tests import decimate_model as dm
from tests import digest_model as dgm
from tests import energy_model as em
from tests import levels_model as lm
from tests import requant_model as qm
from tests import resample_model as rm
from tests import pass_list_cases as plc

K = plc.kernel_constants()
THREADS = K["THREADS"]


def test_the_constants_are_the_headers():
    assert THREADS == 256 == dgm.JOIN
    assert (K["DVDA_CRC_TILE_BYTES"], K["DVDA_LVL_TILE_FRAMES"], K["DVDA_NRG_PIECE_FRAMES"], K["DVDA_DCM_TILE_FRAMES"],
            K["DVDA_RSM_TILE_FRAMES"]) == (dgm.TILE, lm.TILE, em.PIECE, dm.TILE, rm.TILE)
    assert K["DVDA_LVL_TILE_FRAMES"] == qm.TILE and K["DVDA_RSM_TILE_FRAMES"] == K["PAIRS"] * rm.UP
    grids = {name: K["TILE_BLOCKS", name] for name in plc.ALL}
    assert {n for n, g in grids.items() if g == 2048} == {"levels", "compare", "energy", "requantize"}
    assert {n for n, g in grids.items() if g == 4096} == {"digest", "decimate", "resample"}
    assert set(grids.values()) == set(plc.SECOND_RUN)


# ---- part A
def test_resample_reaches_every_chunk_size_and_partial_chunk(pkg):
    """k_rs_tiles takes a tile of PAIRS blocks in chunks of PAIRS / ch blocks: the eight sizes, and the three partial
    last chunks of a full tile; the second tile is neither whole blocks nor whole work items"""
    p = plc.the_pass("resample", 24)
    streams = plc.channel_cases(p)
    assert [s.pcm.shape[0] for s in streams] == list(range(1, 9))
    nb = [K["PAIRS"] // s.pcm.shape[0] for s in streams]
    assert nb == [64, 32, 21, 16, 12, 10, 9, 8]
    assert [K["PAIRS"] % b for b in nb] == [0, 0, 1, 0, 4, 4, 1, 0]
    for s in streams:
        out = rm.out_frames(0, s.pcm.shape[1])
        nm = out - p.out_tile
        assert p.tiles(*s.pcm.shape) == 2 and 0 < nm < p.out_tile and nm % rm.UP and nm % 3
        blocks = -(-nm // rm.UP)
        assert blocks < K["PAIRS"]                      # a tile of fewer blocks: its last chunk is cut by the tile's end
    # ... and for every channel count the second tile is one chunk of fewer blocks than a chunk holds
    assert all(0 < -(-(rm.out_frames(0, s.pcm.shape[1]) - p.out_tile) // rm.UP) < b for s, b in zip(streams, nb))


@pytest.mark.parametrize("D", dm.RATIOS)
def test_decimate_reaches_every_chunk_size_and_both_sides_of_each_step(D):
    """chunk_out(D, ch) over ch = 1 .. 8: at D = 4 all three sizes with the steps between 3 | 4 and 6 | 7 channels, at
    D = 2 the two sizes it has with the step between 6 | 7 (eight channels of 512 fit: 256 is never chosen there)"""
    p = plc.the_pass("decimate", D, 24)
    streams = plc.channel_cases(p)
    chunk = [plc.decim_chunk_out(D, s.pcm.shape[0]) for s in streams]
    assert chunk == {4: [1024] * 3 + [512] * 3 + [256] * 2, 2: [1024] * 6 + [512] * 2}[D]
    assert all(plc.decim_staged_words(D, ch) <= K["LDS_WORDS"] for ch in range(1, 9))
    if D == 4:
        assert plc.decim_staged_words(4, 3) == 14274            # the tightest fit of the largest chunk
    # one channel more at the larger chunk does not fit: each step is forced
    for ch in range(1, 8):
        if chunk[ch] < chunk[ch - 1]:
            assert plc.decim_staged_words(D, ch) // ch * (ch + 1) > K["LDS_WORDS"]
    for s in streams:
        out = dm.out_frames(0, s.pcm.shape[1], D)
        nm = out - p.out_tile
        assert p.tiles(*s.pcm.shape) == 2 and 0 < nm and nm % (K["LANE_SPAN"] // D) and nm % 4
        assert nm % plc.decim_chunk_out(D, s.pcm.shape[0])       # ... and its last chunk is a partial one


def test_requantize_and_energy_second_tiles_are_ragged():
    for bits_out in (16, 24):
        p = plc.the_pass("requantize", bits_out)
        for s in plc.channel_cases(p):
            assert p.tiles(*s.pcm.shape) == 2 and (s.pcm.shape[1] - p.tile) % 4
        assert {s.f0 % 4 for s in plc.channel_cases(p)} == {0, 1, 2, 3}        # every phase of the noise word's quad
    for B, tiles in ((64, None), (4410, 2)):
        p = plc.the_pass("energy", B)
        for s in plc.channel_cases(p):
            frames = s.pcm.shape[1]
            assert p.piece < frames < 4410 and frames % 64
            assert p.tiles(*s.pcm.shape) == (tiles or frames // 64 + 1)


@pytest.mark.parametrize("case", plc.channel_passes(), ids=lambda c: c[0])
def test_channel_cases_lie_at_every_alignment(pkg, case):
    _, p, (lay_in, lay_out) = case
    streams = plc.channel_cases(p)
    assert [s.pcm.shape[0] for s in streams] == list(range(1, 9)) and all(s.kind == "taken" for s in streams)
    st = p.stage(pkg.hipdec, streams, lay_in, lay_out)
    assert {d[0] % 4 for d in st.desc_in} == {0, 1, 2, 3}
    if lay_in == "planar":
        assert {d[1] & 1 for d in st.desc_in if d[3] > 1} == {0, 1}
    if p.writes and lay_out != "wav":
        assert {d[0] % 4 for d in st.desc_out} == {0, 1, 2, 3}
        if lay_out == "planar":
            assert {d[1] & 1 for d in st.desc_out if d[3] > 1} == {0, 1}
    if p.writes:
        assert 0 < sum(sum(r["clipped"]) for r in st.reports)
        assert not np.array_equal(st.start, st.expect)


# ---- part B
@pytest.mark.parametrize("name", plc.ALL)
def test_long_list_premises(name):
    """n above the scan's one-launch form; more tiles than the tile kernel has workgroups (than twice as many, where it
    has 2048); the two runs of two-tile streams a grid apart with other channel counts; the rules of the plain streams;
    the cut behind the first turn and inside a stream"""
    p = plc.list_pass(name)
    streams, info = plc.long_list(p)
    n, g = len(streams), p.grid
    assert n == plc.N_LIST > 4096
    total = int(info.base[-1])
    assert total > g and total > 4096 == max(2 * 2048, 4096) and total > n
    print(name, "n", n, "tiles", total, "turns of a workgroup", -(-total // g), "bulk tiles", info.bulk)
    # the rules
    special = set(range(plc.FIRST_RUN, plc.FIRST_RUN + 8)) | set(range(info.run[1], info.run[1] + 8)) | \
        set(range(plc.BULK_AT, plc.BULK_AT + plc.BULK_N)) | set(range(plc.TAIL_AT, plc.TAIL_AT + plc.TAIL_N))
    kinds = set()
    for i, s in enumerate(streams):
        ch, frames = s.pcm.shape
        assert (frames == 0) == (i % 37 == 0) and (s.kind != "taken") == (i % 50 == 49)
        if s.kind != "taken":
            kinds.add(s.kind)
        if i not in special and frames:
            assert 1 <= frames <= 40 and 1 <= ch <= 8
            assert info.counts[i] == (1 if s.kind == "taken" else 0)
    assert kinds == set(p.untaken)
    assert {s.pcm.shape[0] for i, s in enumerate(streams) if i not in special} == set(range(1, 9))
    assert not any(i % 37 == 0 or i % 50 == 49 for i in special)
    # the runs: list positions b and b + TILE_BLOCKS are both full tiles, of streams with other channel counts
    first, second = info.run
    assert int(info.base[first]) == 0 and int(info.base[second]) == g
    for k in range(8):
        a, b = streams[first + k], streams[second + k]
        assert a.pcm.shape[0] != b.pcm.shape[0]
        for s, i in ((a, first + k), (b, second + k)):
            assert s.pcm.shape[1] == 2 * p.unit(s.pcm.shape[0]) and info.counts[i] == 2
            assert int(info.base[i]) % g == 2 * k
    assert {s.pcm.shape[0] for s in streams[first:first + 8]} == set(p.run_channels)
    # many-tile streams in front of the second run: a stream's tiles go to as many workgroups, in both turns
    assert all(info.counts[plc.BULK_AT + k] == info.bulk for k in range(plc.BULK_N - 1))
    # the cut: inside a stream, behind the first turn of every workgroup
    cut = info.cut
    mt = p.max_tiles(n, info.max_total)
    assert g <= int(info.base[cut]) < mt < int(info.base[cut + 1]) <= total
    assert mt // g >= 1 and info.counts[cut] == p.tail_tiles
    assert any(c for c in info.counts[cut + 1:])


# ---- part C
@pytest.mark.parametrize("name", plc.WRITERS)
def test_long_stream_premises(pkg, name):
    """THREADS + 1 tiles; in the "tail" content the model's count is non-zero and all of it lies in the last tile"""
    hd = pkg.hipdec
    p = plc.list_pass(name)
    for content in ("mixed", "tail"):
        long, short = plc.long_stream(p, content)
        assert long.pcm.shape[0] == 1 and p.tiles(*long.pcm.shape) == THREADS + 1 and p.tiles(*short.pcm.shape) == 1
        assert p.out_frames(long.pcm.shape[1]) == THREADS * p.out_tile + 100
    pcm = long.pcm
    frames = pcm.shape[1]
    loud = plc.LOUD[name]
    assert np.abs(pcm[0, :frames - loud].astype(np.int64)).max() <= plc.QUIET
    if name == "requantize":
        head = qm.requant_np(pcm[:, :THREADS * p.tile], 24, 16, p.mode, plc.SEED, 0)[1]
        whole = p.want(hd, long)[1]["clipped"]
        last = whole
    elif name == "decimate":
        H = dm.half(p.D)
        region, f0, before, after = dm.cut(pcm, 0, p.D * THREADS * p.out_tile, H, H)
        head = dm.decimate_np(np.ascontiguousarray(region), plc.decim_taps(hd, p.D), p.D, p.bits, f0, before, after)[1]
        whole = p.want(hd, long)[1]["clipped"]
        last = whole
    else:
        # (the whole is the GPU file's to compute, tile by tile.)  No output whose window lies in the quiet part can
        # clip: |y| <= QUIET * max sum |g| / 2^30; the loud frames begin more than a window behind the last tile's first
        # input frame, so every output they reach lies in the last tile; that tile alone, as a piece, has the count.
        gain = int(np.abs(plc.resample_table(hd).astype(np.int64)).sum(axis=1).max())
        assert (plc.QUIET * gain >> 30) + 1 < 1 << (p.bits - 1)
        assert frames - loud - 48 > THREADS * p.in_tile
        head = [0] * 8
        last = p.slice_model(hd, pcm, THREADS)[1]
    assert head == [0] * 8 and last[0] > 0 and last[1:] == [0] * 7
    print(name, "clipped, all in tile", THREADS, ":", last[0])


# ---- part D
@pytest.mark.parametrize("name", plc.WRITERS)
def test_every_output_clips(pkg, name):
    """eight channels at the rails of int32, reduced to 16 bits: a full tile's count is the tile, in every field"""
    p = plc.clip_pass(name)
    (s,) = plc.all_clip(p)
    out, report = p.want(pkg.hipdec, s)
    assert out.shape == (8, p.out_tile + 1) and p.tiles(*s.pcm.shape) == 2
    assert report["clipped"] == [p.out_tile + 1] * 8
    assert p.out_tile < 1 << 16
    assert all((out[c] == (-2 ** 15 if c % 2 == 0 else 2 ** 15 - 1)).all() for c in range(8))
