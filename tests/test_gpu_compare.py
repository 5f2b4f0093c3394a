"""The compare of two PCM buffers on the GPU (dvda_pcm_hip_compare, dvda_mlp_hip_pcm_compare; csrc/pcm_compare.h): what
the device reports of two int32 buffers, each in either layout, is tests/compare_model.diff of the same values.  Every
comparison is exact."""
import itertools

import numpy as np
import pytest

from tests import compare_model as cm
from tests.stream_tools import frame_offsets
from tests.test_presentation_model import make_stream

pytestmark = pytest.mark.gpu

T = cm.TILE
LAYOUTS = ["planar", "interleaved"]
PAIRS = list(itertools.product(LAYOUTS, LAYOUTS))
FILL = np.array(0xA5A5A5A5, np.uint32).view(np.int32)[()]       # poison around every region: never part of a report


def _layout(hd, name):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24, "wav16": hd.PCM_WAV16}[name]


def place(pcms, layout, slack, off_mod=None, order=None, declare=None):
    """lays the streams (planar int32 [ch, frames]) out in `layout` in one buffer filled with poison, stream i with
    capacity frames + slack[i] and at an offset = off_mod[i] (mod 4) int32 units; `order`: the sequence in which the
    streams lie in memory (the descriptors stay in the streams' order); declare: (frames, channels) a stream's descriptor
    states instead of its own -> (flat int32 array, desc list)"""
    parts, desc, pos = [np.full(5, FILL, np.int32)], [None] * len(pcms), 5
    for i in (order if order is not None else range(len(pcms))):
        p = pcms[i]
        ch, frames = p.shape
        stride = frames + slack[i % len(slack)]
        if off_mod is not None:
            pad = (off_mod[i % len(off_mod)] - pos) % 4
            parts.append(np.full(pad, FILL, np.int32))
            pos += pad
        if layout == "planar":
            region = np.full((ch, stride), FILL, np.int32)
            region[:, :frames] = p
        else:
            region = np.full((stride, ch), FILL, np.int32)
            region[:frames] = p.T
        desc[i] = (pos, stride) + ((frames, ch) if declare is None or declare[i] is None else declare[i])
        parts.append(region.reshape(-1))
        pos += region.size
    parts.append(np.full(7, FILL, np.int32))
    return np.concatenate(parts), desc


def run(hd, flat_a, la, desc_a, flat_b, lb, desc_b, bits, **kw):
    import torch
    dev = torch.device("cuda", 0)
    d_a, d_b = torch.from_numpy(flat_a).to(dev), torch.from_numpy(flat_b).to(dev)
    return hd.diff_list(hd.pcm_compare(d_a, _layout(hd, la), desc_a, d_b, _layout(hd, lb), desc_b, bits, **kw))


def check(hd, pa, pb, la, lb, bits, slack=(0, 1, 2), slack_b=None, kw_a=None, kw_b=None):
    flat_a, desc_a = place(pa, la, slack, **(kw_a or {}))
    flat_b, desc_b = place(pb, lb, slack[::-1] if slack_b is None else slack_b, **(kw_b or {}))
    got = run(hd, flat_a, la, desc_a, flat_b, lb, desc_b, bits)
    want = [cm.diff(a, b, bits) for a, b in zip(pa, pb)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, pa[i].shape, pb[i].shape, desc_a[i], desc_b[i])
    return want, desc_a, desc_b


def random_pair(rng, ch, fa, fb=None, share=0.02):
    """random int32 [ch, fa] and [ch, fb]: B is A (as far as both go) except for a `share` of the values"""
    fb = fa if fb is None else fb
    a = rng.integers(-2 ** 31, 2 ** 31, (ch, fa), dtype=np.int64).astype(np.int32)
    b = rng.integers(-2 ** 31, 2 ** 31, (ch, fb), dtype=np.int64).astype(np.int32)
    n = min(fa, fb)
    keep = rng.random((ch, n)) >= share
    b[:, :n][keep] = a[:, :n][keep]
    return a, b


@pytest.mark.parametrize("ch", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("bits", [0, 16, 24])
@pytest.mark.parametrize("la,lb", PAIRS)
def test_sweep(pkg, la, lb, bits, ch):
    rng = np.random.default_rng(1000 * ch + bits + 7 * len(la) + len(lb))
    frames = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]
    pairs = [random_pair(rng, ch, f) for f in frames]
    want, _, _ = check(pkg.hipdec, [a for a, _ in pairs], [b for _, b in pairs], la, lb, bits)
    assert 0 < want[-1]["diff_frames"] < frames[-1] and want[-1]["runs"] > 1


@pytest.mark.parametrize("bits", [0, 16])
@pytest.mark.parametrize("la,lb", PAIRS)
def test_alignment_and_order(pkg, la, lb, bits):
    """off mod 4 of A and of B independently: all 16 combinations over the batch; odd planar strides; the streams of one
    side shuffled in memory"""
    rng = np.random.default_rng(77 + bits)
    chans = [2, 3, 6, 1, 5, 2, 3, 1, 6, 4, 8, 7, 6, 2, 3, 5]
    frames = [3 * T + 7, 5, 700, T + 1, 2, T - 1, 10000, 2 * T, 3, T + 2, 700, 2 * T + 3, 513, 64, 1365, 820]
    pairs = [random_pair(rng, c, f) for c, f in zip(chans, frames)]
    slack = [37 + (f & 1) for f in frames]              # planar: every stride is odd
    order = [7, 2, 11, 0, 15, 5, 9, 13, 1, 10, 3, 12, 8, 6, 14, 4]
    _, desc_a, desc_b = check(pkg.hipdec, [a for a, _ in pairs], [b for _, b in pairs], la, lb, bits, slack=slack, slack_b=slack,
                              kw_a=dict(off_mod=[i % 4 for i in range(16)]),
                              kw_b=dict(off_mod=[i // 4 for i in range(16)], order=order))
    assert {(x[0] % 4, y[0] % 4) for x, y in zip(desc_a, desc_b)} == set(itertools.product(range(4), range(4)))
    assert [d[0] for d in desc_b] != sorted(d[0] for d in desc_b) and [d[0] for d in desc_a] == sorted(d[0] for d in desc_a)
    for lay, desc in ((la, desc_a), (lb, desc_b)):
        assert lay != "planar" or all(d[1] & 1 for d in desc)


@pytest.mark.parametrize("la,lb", PAIRS)
def test_one_value(pkg, la, lb):
    ch, frames = 3, 3 * T + 7
    a = random_pair(np.random.default_rng(4), ch, frames)[0]
    places = [0, frames - 1, T - 1, T, frames // 2]
    others = []
    for at in places:
        b = a.copy()
        b[ch - 1, at] ^= 0x100                  # one value, in the last channel only
        others.append(b)
    want, _, _ = check(pkg.hipdec, [a] * len(places), others, la, lb, 0, slack=(2,))
    for at, w in zip(places, want):
        assert w["diff_frames"] == w["runs"] == 1 and w["first_diff"] + 1 == w["diff_end"] == at + 1
        assert w["diff_values"] == [0, 0, 1, 0, 0, 0, 0, 0] and w["max_abs"][2] == 0x100


@pytest.mark.parametrize("la,lb", PAIRS)
def test_runs_at_tile_seams(pkg, la, lb):
    ch, frames = 2, 3 * T + 7
    a = random_pair(np.random.default_rng(5), ch, frames)[0]

    def other(idx):
        b = a.copy()
        b[1, idx] = ~b[1, idx]
        return b

    masks = [[T - 1, T], [T - 1, T + 1], np.arange(T, 2 * T), np.arange(frames), np.arange(0, frames, 2),
             np.arange(T - 64, T + 64), [T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1]]
    want, _, _ = check(pkg.hipdec, [a] * len(masks), [other(m) for m in masks], la, lb, 0, slack=(1,))
    assert [w["runs"] for w in want] == [1, 2, 1, 1, (frames + 1) // 2, 1, 3]
    assert [w["diff_frames"] for w in want] == [2, 2, T, frames, (frames + 1) // 2, 128, 5]
    assert want[4]["compared"] // 2 == want[4]["runs"] - 1 and frames % 2 == 1      # (odd length: one more than half)
    assert (want[2]["first_diff"], want[2]["diff_end"]) == (T, 2 * T)
    # an even length: runs is compared / 2
    even = check(pkg.hipdec, [a[:, :2 * T]], [other(np.arange(1, 2 * T, 2))[:, :2 * T]], la, lb, 0)[0][0]
    assert even["runs"] == even["compared"] // 2 == T


@pytest.mark.parametrize("bits", [0, 16, 20, 24])
@pytest.mark.parametrize("la,lb", PAIRS)
def test_rails_and_bits(pkg, la, lb, bits):
    """the known values of tests/test_compare_model.py, and a channel that holds only -2^31 against 2^31 - 1"""
    known = [(40000, 7232), (-40000, -7232), (5, 5 + 65536), (-2 ** 31, 2 ** 31 - 1), (2 ** 23, -2 ** 23), (-1, 2 ** 19 - 1),
             (7, 7)]
    pa, pb = [], []
    for frames in (len(known), T + len(known)):
        a, b = np.zeros((3, frames), np.int64), np.zeros((3, frames), np.int64)
        a[0], b[0] = -2 ** 31, 2 ** 31 - 1              # a channel of nothing but the two rails
        a[1, -len(known):] = [x for x, _ in known]      # every known pair once, at the stream's end
        b[1, -len(known):] = [y for _, y in known]
        pa.append(a.astype(np.int32))
        pb.append(b.astype(np.int32))
    want, _, _ = check(pkg.hipdec, pa, pb, la, lb, bits, slack=(3,))
    for w in want:
        if bits == 0:
            assert w["max_abs"][:3] == [2 ** 32 - 1, 2 ** 32 - 1, 0] and w["diff_frames"] == w["compared"]
            assert w["diff_values"][1] == 6
        else:
            # -2^31 is written as -2^(bits-1), 2^31 - 1 as 2^(bits-1) - 1: a full-scale difference
            assert w["max_abs"][0] == 2 ** bits - 1 and w["diff_values"][0] == w["compared"]
    if bits == 16:
        # the first three pairs give the same sample; the rails, (2^23, -2^23): 0 and -2^15, (-1, 2^19 - 1): -1 and 2^15 - 1
        assert want[0]["diff_values"][1] == 3 and want[0]["max_abs"][1] == 2 ** 16 - 1
    if bits == 24:
        assert want[0]["diff_values"][1] == 6 and want[0]["max_abs"][1] == 2 ** 24 - 1


@pytest.mark.parametrize("la,lb", PAIRS)
def test_shapes(pkg, la, lb):
    """unequal lengths both ways -- the longer side's tail is poison that must not show -- and descriptors that do not go
    together"""
    hd = pkg.hipdec
    rng = np.random.default_rng(6)
    a0, b0 = random_pair(rng, 3, T + 9, T + 9)
    a1, b1 = random_pair(rng, 2, 3 * T + 7, 3 * T + 7)
    pa = [a0, a1[:, :T + 1], a0, a0[:2], np.zeros((8, 5), np.int32), a0[:1, :100]]
    pb = [b0[:, :70], b1, b0[:2], b0, np.zeros((8, 5), np.int32), b0[:1, :0]]
    # the longer side's tail: poison in the buffer, and declared as frames
    for p, q in ((pa, pb), (pb, pa)):
        for i in (0, 1):
            if p[i].shape[1] > q[i].shape[1]:
                p[i] = p[i].copy()
                p[i][:, q[i].shape[1]:] = FILL
    declare = [None] * 4 + [(5, 9), None]       # a 9-channel descriptor (over an 8-channel region)
    flat_a, desc_a = place(pa, la, (1,), declare=declare)
    flat_b, desc_b = place(pb, lb, (2,), declare=declare)
    got = run(hd, flat_a, la, desc_a, flat_b, lb, desc_b, 0)
    want = [cm.diff(a, b, 0) for a, b in zip(pa, pb)]
    want[4] = dict(cm.zero(), flags=cm.CMP_SHAPE)
    assert got == want
    assert [g["compared"] for g in got] == [70, T + 1, 0, 0, 0, 0] and [g["flags"] for g in got] == [0, 0, 1, 1, 1, 0]
    assert (got[0]["frames_a"], got[0]["frames_b"]) == (T + 9, 70) and (got[5]["frames_a"], got[5]["channels"]) == (100, 1)
    # no pairs at all
    import torch
    z = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    assert hd.diff_list(hd.pcm_compare(z, _layout(hd, la), [], z, _layout(hd, lb), [])) == []


@pytest.mark.parametrize("la,lb", PAIRS)
def test_bound_too_small_reads_nothing_wrong(pkg, la, lb):
    """a pair whose tiles fall outside max_total_frames is reported as zeros; the pairs inside it are right"""
    hd = pkg.hipdec
    rng = np.random.default_rng(10)
    pairs = [random_pair(rng, 2, T), random_pair(rng, 2, 4 * T), random_pair(rng, 1, 5)]        # 1, 4 and 1 tiles
    flat_a, desc_a = place([a for a, _ in pairs], la, (0,))
    flat_b, desc_b = place([b for _, b in pairs], lb, (0,))
    got = run(hd, flat_a, la, desc_a, flat_b, lb, desc_b, 0, max_total_frames=T)                # room for 1 + 3 tiles
    assert got == [cm.diff(*pairs[0], 0), cm.zero(), cm.zero()]
    assert got[0]["diff_frames"] > 0


@pytest.mark.parametrize("la,lb", PAIRS)
def test_deterministic_on_a_poisoned_workspace(pkg, la, lb):
    import torch
    hd = pkg.hipdec
    rng = np.random.default_rng(9)
    pairs = [random_pair(rng, c, f, share=0.3) for c, f in ((2, 9000), (6, 0), (3, 17), (1, 30000), (6, 5000))]
    flat_a, desc_a = place([a for a, _ in pairs], la, (1,))
    flat_b, desc_b = place([b for _, b in pairs], lb, (1,))
    dev = torch.device("cuda", 0)
    d_a, d_b = torch.from_numpy(flat_a).to(dev), torch.from_numpy(flat_b).to(dev)
    total = sum(a.shape[1] for a, _ in pairs)
    work = torch.empty(hd.pcm_compare_workspace_words(len(pairs), total), dtype=torch.int32, device=dev)
    raw = []
    for poison in (-1, 0x5A5A5A5A):
        work.fill_(poison)
        out = hd.pcm_compare(d_a, _layout(hd, la), desc_a, d_b, _layout(hd, lb), desc_b, 0, work=work)
        raw.append(out.cpu().numpy().tobytes())
    assert raw[0] == raw[1]
    assert hd.diff_list(out) == [cm.diff(a, b, 0) for a, b in pairs]


_MANY = []


@pytest.mark.parametrize("la,lb", [("planar", "planar"), ("interleaved", "interleaved"), ("planar", "interleaved")])
def test_many_tiles(pkg, la, lb):
    """more tiles than the tile kernel has workgroups, a pair with more tiles than a join workgroup has threads"""
    if not _MANY:
        rng = np.random.default_rng(300)
        _MANY.append(random_pair(rng, 1, 257 * T + 1))
        _MANY.extend(random_pair(rng, int(rng.integers(1, 3)), int(rng.integers(0, 20 * T))) for _ in range(190))
    pairs = _MANY
    assert sum(-(-a.shape[1] // T) for a, _ in pairs) > 2048
    check(pkg.hipdec, [a for a, _ in pairs], [b for _, b in pairs], la, lb, 0, slack=(0, 3))


@pytest.mark.parametrize("layout", ["wav24", "wav16"])
def test_wav_layouts_are_refused(pkg, layout):
    import torch
    hd = pkg.hipdec
    z = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    desc = [(0, 8, 8, 1)]
    for la, lb in ((layout, "planar"), ("interleaved", layout)):
        with pytest.raises(hd.HipError, match="EINVAL"):
            hd.pcm_compare(z, _layout(hd, la), desc, z, _layout(hd, lb), desc)
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.pcm_compare(z, 0, desc, z, 1, desc, bits=8)


_STREAMS = {}


def mixed_streams(pkg):
    """8 streams of the generator: one and two substreams, 2 and 6 channels, plain and chained, under and over a tile"""
    if not _STREAMS:
        kinds = [(0, 12, 2, 48), ("CHAINED", 12, 2, 60), ("DISC|CHAINED", 12, 2, 48), (0, 12, 1, 60), ("CHAINED", 1, 1, 48),
                 (0, 1, 1, 7), ("CHAINED", 12, 1, 60), (0, 12, 2, 3)]
        _STREAMS["b"] = [make_stream(pkg, feat, seed, assignment=asg, S=S, n_aus=n)[0]
                         for seed, (feat, asg, S, n) in enumerate(kinds)]
    return _STREAMS["b"]


def test_behind_a_decode(pkg):
    """a batch decoded planar on one context and frame-major on another: the same samples"""
    hd = pkg.hipdec
    streams = mixed_streams(pkg)
    sides = []
    try:
        for layout in (hd.PCM_PLANAR, hd.PCM_INTERLEAVED):
            batch = hd.Batch(streams)
            ctx = hd.Context(0, batch.n, max(64, batch.total // 64), 0, layout)
            sides.append((ctx, batch))
            regions, infos, _ = hd.decode_batch(ctx, batch, layout, attempts=2, to_host=False)
            assert isinstance(regions, hd.PcmRegions) and not any(inf.status & ~hd.ST_BENIGN for inf in infos)
            sides[-1] = (ctx, batch, regions, infos)
        (ctx_a, batch_a, reg_a, infos_a), (ctx_b, batch_b, reg_b, infos_b) = sides
        desc_b = [(o, r, int(inf.pcm_frames), int(inf.channels)) for o, r, inf in zip(reg_b.out_off, reg_b.rows, infos_b)]
        desc_a = [(o, r, int(inf.pcm_frames), int(inf.channels)) for o, r, inf in zip(reg_a.out_off, reg_a.rows, infos_a)]
        for bits in (0, 24):
            for got in (ctx_a.pcm_compare(*reg_a.ptrs, reg_b.d_pcm, hd.PCM_INTERLEAVED, desc_b, bits),
                        ctx_b.pcm_compare(*reg_b.ptrs, reg_a.d_pcm, hd.PCM_PLANAR, desc_a, bits)):
                assert len(got) == len(streams)
                for g, inf in zip(got, infos_a):
                    assert g["diff_frames"] == 0 and g["compared"] == int(inf.pcm_frames) > 0 and g["flags"] == 0
                    assert g["channels"] == int(inf.channels) and g["first_diff"] == g["compared"] and g["runs"] == 0
        assert max(int(inf.pcm_frames) for inf in infos_a) > T > min(int(inf.pcm_frames) for inf in infos_a)
        assert {int(inf.channels) for inf in infos_a} == {2, 6}
        # a WAV context is refused
        ctx_a.set_pcm_layout(hd.PCM_WAV24)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx_a.pcm_compare(*reg_a.ptrs, reg_b.d_pcm, hd.PCM_INTERLEAVED, desc_b)
    finally:
        for side in sides:
            side[0].close()


@pytest.mark.parametrize("la,lb", [("interleaved", "interleaved"), ("planar", "interleaved")])
def test_two_rips_one_damaged(pkg, la, lb):
    """compare_streams in conceal mode: one copy damaged in one access unit -- every diff is the model's diff of the two
    host copies, the damaged stream's differing range is not empty, every other stream is clean"""
    hd = pkg.hipdec
    streams = mixed_streams(pkg)
    hurt = 1
    offs = frame_offsets(streams[hurt])
    bad = streams[hurt].copy()
    bad[offs[19] + (offs[20] - offs[19]) // 2] ^= 0x10
    other = [bad if i == hurt else s for i, s in enumerate(streams)]
    infos_a, infos_b, diffs = hd.compare_streams(streams, other, layout_a=_layout(hd, la), layout_b=_layout(hd, lb),
                                                 conceal=True)
    pcm_a = hd.decode_streams_concealed(streams, layout=_layout(hd, la))[0]
    pcm_b, _, spans = hd.decode_streams_concealed(other, layout=_layout(hd, lb))
    assert infos_b[hurt].status & hd.ST_CONCEALED and spans[hurt] and not infos_a[hurt].status & hd.ST_CONCEALED
    assert diffs == [cm.diff(a, b, 0) for a, b in zip(pcm_a, pcm_b)]
    for i, d in enumerate(diffs):
        assert d["compared"] == min(int(infos_a[i].pcm_frames), int(infos_b[i].pcm_frames)) > 0
        if i == hurt:
            assert d["first_diff"] < d["diff_end"] and d["diff_frames"] > 0 and d["runs"] >= 1
        else:
            assert d["diff_frames"] == 0 and d["diff_end"] == 0 and d["frames_a"] == d["frames_b"]
    assert len(hd.compare_streams(streams[:2], streams[:2])) == 3
