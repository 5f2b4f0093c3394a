"""The channel mix on the GPU (dvda_pcm_hip_mix; csrc/pcm_mix.h): what the device writes -- int32 PCM of the matrix's
output channels in either layout -- and what it counts is tests/mix_model of the same values; nothing else in the output
buffer or around the workspace changes.  Every comparison is exact."""
import numpy as np
import pytest

from tests import mix_model as mm
from tests.test_gpu_levels import FILL, LAYOUTS, _layout, place

pytestmark = pytest.mark.gpu

T = mm.TILE
THREADS = 256                   # pcmt::THREADS: a join workgroup sums that many tiles per turn
RAGGED = 2 * T + 2501           # two tiles and a third of two chunks and 453 frames: no multiple of a lane's 4 or a chunk
FRAMES = [0, 1, T - 1, T, T + 1, RAGGED]
PAIRS = sorted({(i, o) for i in range(1, 9) for o in (1, 2, i)} | {(6, 8), (1, 8)})
LO, HI = -2 ** 31, 2 ** 31 - 1
_PCM, _MAT, _WANT = {}, {}, {}


def pcm_of(ch, frames, bits=24):
    """computed once, shared, never written to: a quarter over the whole of int32, the rest inside `bits`"""
    key = (ch, frames, bits)
    if key not in _PCM:
        rng = np.random.default_rng(7000 * ch + frames + bits)
        p = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (ch, frames), dtype=np.int64)
        q = frames // 4
        p[:, :q] = rng.integers(LO, HI + 1, (ch, q), dtype=np.int64)
        p[:, q:q + 2] = [[LO, HI][:max(min(2, frames - q), 0)]] * ch
        _PCM[key] = p.astype(np.int32)
        _PCM[key].setflags(write=False)
    return _PCM[key]


def matrix_of(ich, och, k=0):
    """a random valid matrix, coefficients of both signs, its rows 0 and 3 at sum |coef| = 2^31"""
    key = (ich, och, k)
    if key not in _MAT:
        _MAT[key] = mm.random_matrix(np.random.default_rng(100 * ich + 10 * och + k), ich, och, full_rows=(0, 3))
    return _MAT[key]


def want_of(ich, och, frames, bits, k=0):
    key = (ich, och, frames, bits, k)
    if key not in _WANT:
        out, cl = mm.mix_np(pcm_of(ich, frames, bits), matrix_of(ich, och, k), bits)
        out.setflags(write=False)
        _WANT[key] = (out, cl)
    return _WANT[key]


def blank(flat, d, layout, och):
    """the region of descriptor d (as place cut it for och channels) back to poison: a stream that writes nothing"""
    off, stride, frames, _ = d
    flat[off:off + stride * och] = FILL


def run(hd, flat_in, layout_in, desc_in, mats, bits, flat_want, layout_out, desc_out, **kw):
    """the call on an output buffer of poison -> (the buffer afterwards, reports); the input is read only"""
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(flat_in).to(dev)
    d_out = torch.from_numpy(np.full_like(flat_want, FILL)).to(dev)
    got, desc, d_rep = hd.pcm_mix(d_in, _layout(hd, layout_in), desc_in, mats, bits, out=d_out,
                                  layout_out=_layout(hd, layout_out), desc_out=desc_out, **kw)
    assert got is d_out and desc is desc_out
    reports = hd.mix_list(d_rep)
    assert np.array_equal(d_in.cpu().numpy(), flat_in)
    return d_out.cpu().numpy(), reports


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("bits", mm.DEPTHS)
@pytest.mark.parametrize("layout_out", LAYOUTS)
@pytest.mark.parametrize("layout_in", LAYOUTS)
def test_sweep(pkg, layout_in, layout_out, bits):
    """every pair of channel counts and every length in one call; input and output off at each of the four dword
    alignments, each on its own cycle; planar strides odd and even"""
    hd = pkg.hipdec
    shapes = [(i, o, f) for i, o in PAIRS for f in FRAMES]
    pcms = [pcm_of(i, f, bits) for i, o, f in shapes]
    mats = [matrix_of(i, o) for i, o, f in shapes]
    want = [want_of(i, o, f, bits) for i, o, f in shapes]
    flat_in, desc_in = place(pcms, layout_in, [37, 38, 40, 35], off_mod=[0, 1, 2, 3, 3, 2, 1])
    flat_want, desc_out = place([w for w, _ in want], layout_out, [11, 12, 9, 16, 10], off_mod=[2, 0, 3, 1, 1])
    assert len({(a[0] % 4, b[0] % 4) for a, b in zip(desc_in, desc_out)}) == 16
    assert {d[1] & 1 for d in desc_in} == {0, 1} == {d[1] & 1 for d in desc_out}
    got, reports = run(hd, flat_in, layout_in, desc_in, mats, bits, flat_want, layout_out, desc_out)
    for k, (i, o, f) in enumerate(shapes):
        assert reports[k] == mm.report(f, want[k][1]), (k, i, o, f)
    same(got, flat_want)
    clipped = sum(sum(r["clipped"]) for r in reports)
    assert 0 < clipped < sum(o * f for i, o, f in shapes)


@pytest.mark.parametrize("layout_out", LAYOUTS)
@pytest.mark.parametrize("layout_in", LAYOUTS)
def test_identity_permutation_extraction(pkg, layout_in, layout_out):
    """2^30 on the diagonal copies values inside `bits` bit for bit; rows of one 2^30 permute or extract"""
    hd = pkg.hipdec
    rng = np.random.default_rng(3)
    pcms, mats, want = [], [], []
    for ch in range(1, 9):
        p = rng.integers(-(1 << 23), 1 << 23, (ch, T + 1 + 97 * ch), dtype=np.int64).astype(np.int32)
        p[:, :2] = [[-(1 << 23), (1 << 23) - 1]] * ch
        perm = [int(v) for v in rng.permutation(ch)]
        pick = int(rng.integers(ch))
        for m, w in ((mm.identity(ch), p), (mm.matrix(ch, ch, [[mm.ONE if c == perm[o] else 0 for c in range(ch)]
                                                               for o in range(ch)]), p[perm]),
                     (mm.matrix(ch, 1, [[mm.ONE if c == pick else 0 for c in range(ch)]]), p[pick:pick + 1])):
            pcms.append(p)
            mats.append(m)
            want.append(w)
    flat_in, desc_in = place(pcms, layout_in, [5, 6], off_mod=[1, 0, 3, 2])
    flat_want, desc_out = place(want, layout_out, [3, 8], off_mod=[0, 3, 1, 2, 2])
    got, reports = run(hd, flat_in, layout_in, desc_in, mats, 24, flat_want, layout_out, desc_out)
    same(got, flat_want)
    assert reports == [mm.report(p.shape[1], [0] * 8) for p in pcms]


@pytest.mark.parametrize("layout_out", LAYOUTS)
def test_count_fields_at_their_maximum(pkg, layout_out):
    """eight output channels, every value of full tiles clipped: each 16-bit field of both count words at TILE"""
    hd = pkg.hipdec
    pcm = np.empty((8, 2 * T), np.int32)
    pcm[:, 0::2], pcm[:, 1::2] = LO, HI
    m = mm.matrix(8, 8, [[(-1) ** o * mm.ONE if c == o else 0 for c in range(8)] for o in range(8)])
    want, cl = mm.mix_np(pcm, m, 16)
    assert cl == [2 * T] * 8
    for layout_in in LAYOUTS:
        flat_in, desc_in = place([pcm], layout_in, [0], off_mod=[0])
        flat_want, desc_out = place([want], layout_out, [0], off_mod=[0])
        got, reports = run(hd, flat_in, layout_in, desc_in, [m], 16, flat_want, layout_out, desc_out)
        same(got, flat_want)
        assert reports == [mm.report(2 * T, cl)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_more_tiles_than_a_join_turn(pkg, layout):
    """a stream of THREADS + 1 tiles whose only clipped values lie in the last tile"""
    hd = pkg.hipdec
    frames = THREADS * T + 77
    rng = np.random.default_rng(17)
    pcm = rng.integers(-(1 << 14), 1 << 14, (2, frames), dtype=np.int64).astype(np.int32)
    pcm[0, THREADS * T + 5:THREADS * T + 9] = HI
    pcm[1, frames - 1] = LO
    m = mm.matrix(2, 2, [[mm.ONE, 0], [mm.HALF, mm.HALF]])
    want, cl = mm.mix_np(pcm, m, 16)
    assert cl[0] == 4 and cl[1] >= 1 and mm.mix_np(pcm[:, :THREADS * T], m, 16)[1] == [0] * 8
    assert (frames + T - 1) // T == THREADS + 1
    flat_in, desc_in = place([pcm], layout, [3], off_mod=[1])
    flat_want, desc_out = place([want], layout, [5], off_mod=[3])
    got, reports = run(hd, flat_in, layout, desc_in, [m], 16, flat_want, layout, desc_out)
    same(got, flat_want)
    assert reports == [mm.report(frames, cl)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_streams_not_taken_write_nothing(pkg, layout):
    hd = pkg.hipdec
    f = T + 300
    half = 1 << 30
    ok = matrix_of(3, 2)
    pcms = [pcm_of(3, f)] * 9
    mats = [ok] * 9
    mats[1] = mm.matrix(4, 2, ok["coef"])                           # in_channels != the descriptor's
    mats[2] = mm.matrix(3, 1, ok["coef"])                           # out_channels != the output descriptor's
    mats[3] = mm.matrix(3, 2, [[half, half, 1], [0, 0, 0]])         # a row at 2^31 + 1
    want, cl = want_of(3, 2, f, 24)
    flat_in, desc_in = place(pcms, layout, [7, 4], off_mod=[0, 1, 2, 3])
    flat_want, desc_out = place([want] * 9, layout, [9, 6], off_mod=[3, 2, 1, 0])
    for k in range(1, 8):
        blank(flat_want, desc_out[k], layout, 2)
    desc_in[4] = desc_in[4][:3] + (0,)                              # channels 0 ...
    desc_in[5] = desc_in[5][:3] + (9,)                              # ... and 9
    desc_out[6] = desc_out[6][:2] + (f - 1, 2)                      # an output descriptor one frame short
    desc_out[7] = (desc_out[7][0], f - 1, f, 2)                     # a stride below its frames
    got, reports = run(hd, flat_in, layout, desc_in, mats, 24, flat_want, layout, desc_out)
    same(got, flat_want)
    assert reports == [mm.report(f, cl)] + [mm.NOT_TAKEN] * 7 + [mm.report(f, cl)]


def many_streams(n=1100):
    """short streams with differing matrices and channel counts, every 37th empty"""
    rng = np.random.default_rng(23)
    shapes = []
    for k in range(n):
        i, o = PAIRS[k % len(PAIRS)]
        shapes.append((i, o, 0 if k % 37 == 0 else int(rng.integers(1, 700))))
    return shapes


@pytest.mark.parametrize("layout_in,layout_out", [("planar", "interleaved"), ("interleaved", "planar")])
def test_a_list_of_1100_streams_on_an_exact_workspace(pkg, layout_in, layout_out):
    """more than 1024 streams: the scan's three-launch form; the workspace exactly *_workspace_words between canaries,
    filled with 0xFF and with 0"""
    import torch
    hd = pkg.hipdec
    shapes = many_streams()
    pcms = [pcm_of(i, f, 20) for i, o, f in shapes]
    mats = [matrix_of(i, o, k % 5) for k, (i, o, f) in enumerate(shapes)]
    want = [mm.mix_np(p, m, 20) for p, m in zip(pcms, mats)]
    flat_in, desc_in = place(pcms, layout_in, [3, 4], off_mod=[0, 1, 2, 3, 3, 2, 1])
    flat_want, desc_out = place([w for w, _ in want], layout_out, [2, 5, 1], off_mod=[2, 0, 3, 1, 1])
    total = sum(f for _, _, f in shapes)
    words = hd.pcm_mix_workspace_words(len(shapes), total)
    for fill in (-1, 0):
        full = torch.full((words + 64,), fill, dtype=torch.int32, device="cuda:0")
        full[:32] = 0x5A5A5A5A
        full[32 + words:] = 0x5A5A5A5A
        got, reports = run(hd, flat_in, layout_in, desc_in, mats, 20, flat_want, layout_out, desc_out,
                           max_total_frames=total, work=full[32:32 + words])
        same(got, flat_want)
        assert reports == [mm.report(f, cl) for (_, _, f), (_, cl) in zip(shapes, want)]
        edge = full.cpu().numpy()
        assert (edge[:32] == 0x5A5A5A5A).all() and (edge[32 + words:] == 0x5A5A5A5A).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_bound_that_cuts_a_stream_in_its_middle(pkg, layout):
    """the streams in front of the cut are mixed; the one it cuts and the ones behind it report zeros, and nothing
    outside their regions is written"""
    hd = pkg.hipdec
    shapes = [(6, 2, 2 * T + 9), (5, 1, 9 * T + 1), (2, 2, T + 3)]
    pcms = [pcm_of(i, f) for i, o, f in shapes]
    mats = [matrix_of(i, o) for i, o, f in shapes]
    want = [want_of(i, o, f, 24) for i, o, f in shapes]
    flat_in, desc_in = place(pcms, layout, [3], off_mod=[1, 2, 3])
    flat_want, desc_out = place([w for w, _ in want], layout, [5], off_mod=[3, 0, 1])
    bound = 4 * T                               # 4 + 3 tiles in the list: the first stream's 3 and 4 of the second's 10
    got, reports = run(hd, flat_in, layout, desc_in, mats, 24, flat_want, layout, desc_out, max_total_frames=bound)
    assert reports == [mm.report(shapes[0][2], want[0][1]), mm.NOT_TAKEN, mm.NOT_TAKEN]
    # (inside the two regions: unspecified values)
    for k in (1, 2):
        off, stride, frames, och = desc_out[k]
        got[off:off + stride * och] = flat_want[off:off + stride * och]
    same(got, flat_want)


@pytest.mark.parametrize("layout_in,layout_out", [("planar", "planar"), ("interleaved", "interleaved"),
                                                  ("planar", "interleaved")])
def test_two_pieces_are_the_whole(pkg, layout_in, layout_out):
    """the pass is pointwise in the frame: a track cut anywhere gives the whole track's bytes, and the reports add"""
    hd = pkg.hipdec
    ich, och, f = 6, 2, 3 * T + 777
    pcm, m = pcm_of(ich, f), matrix_of(ich, och)
    want, cl = want_of(ich, och, f, 24)
    flat_in, desc_in = place([pcm], layout_in, [6], off_mod=[1])
    flat_want, desc_out = place([want], layout_out, [4], off_mod=[2])
    whole, rep = run(hd, flat_in, layout_in, desc_in, [m], 24, flat_want, layout_out, desc_out)
    same(whole, flat_want)
    assert rep == [mm.report(f, cl)]

    def cut(d, layout, a):
        off, stride, frames, ch = d
        step = a if layout == "planar" else a * ch
        return [(off, stride, a, ch), (off + step, stride - (0 if layout == "planar" else a), frames - a, ch)]

    for a in (1, T - 3, T + 1022, f - 1):
        got, reps = run(hd, flat_in, layout_in, cut(desc_in[0], layout_in, a), [m, m], 24, flat_want, layout_out,
                        cut(desc_out[0], layout_out, a))
        same(got, flat_want)
        assert mm.add_reports(*reps) == rep[0] and [r["frames"] for r in reps] == [a, f - a]
