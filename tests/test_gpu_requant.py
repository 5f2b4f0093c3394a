"""The word-length reduction on the GPU (dvda_pcm_hip_requantize, dvda_mlp_hip_pcm_requantize; csrc/pcm_requant.h): what
the device writes -- int32 PCM in either layout or the WAV payload -- and what it counts is tests/requant_model of the
same values; nothing else in the output buffer changes.  Every comparison is exact."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import levels_model as lm
from tests import requant_model as rm
from tests.test_gpu_energy import rail_pcm
from tests.test_gpu_levels import FILL, LAYOUTS, _layout, place

pytestmark = pytest.mark.gpu

T = rm.TILE
CHANNELS = [1, 2, 3, 6, 8]
FRAMES = [1, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
SHAPES = [(ch, f) for ch in CHANNELS for f in FRAMES]
FRAME0 = [0, 1, 2, 3, 2 ** 40 - 5, 12345]
DEPTHS = [(24, 16), (24, 20), (20, 16), (24, 24), (16, 16)]
MODES = [rm.TRUNCATE, rm.ROUND, rm.TPDF]
SEED = 0xDEADBEEFCAFEF00D
OUTS = ["planar", "interleaved", "wav"]
_PCM, _WANT = {}, {}


def mixed_pcm(rng, ch, frames, bits_in):
    """full-range int32 with runs at both rails; the middle half inside the nominal range of bits_in and the last
    quarter inside 24 bits, so that most values do not clip"""
    pcm = rail_pcm(rng, ch, frames).astype(np.int64)
    a, b = frames // 4, frames - frames // 4
    pcm[:, a:b] = rng.integers(-(1 << (bits_in - 1)), 1 << (bits_in - 1), (ch, b - a), dtype=np.int64)
    pcm[:, b:] = rng.integers(-(1 << 23), 1 << 23, (ch, frames - b), dtype=np.int64)
    return pcm.astype(np.int32)


def sweep_pcm(ch, frames, bits_in):
    """computed once, shared, never written to"""
    key = (ch, frames, bits_in)
    if key not in _PCM:
        _PCM[key] = mixed_pcm(np.random.default_rng(1000 * ch + frames + bits_in), ch, frames, bits_in)
        _PCM[key].setflags(write=False)
    return _PCM[key]


def want_of(ch, frames, bits_in, bits_out, mode, frame0):
    key = (ch, frames, bits_in, bits_out, mode, frame0)
    if key not in _WANT:
        out, cl = rm.requant_np(sweep_pcm(ch, frames, bits_in), bits_in, bits_out, mode, SEED, frame0)
        out.setflags(write=False)
        _WANT[key] = (out, cl)
    return _WANT[key]


def place_wav(pcms, bits, gaps=(1, 2, 3), slack=5):
    """the payloads of `pcms` at `bits` in one buffer of poison, stream i from byte 4 * off on with a few words of poison
    behind its last (ragged) dword -> (flat int32 array, desc list)"""
    words, desc, pos = [np.full(3, FILL, np.int32)], [], 3
    for i, p in enumerate(pcms):
        ch, frames = p.shape
        pay = np.frombuffer(rm.payload(p, bits), np.uint8)
        region = np.full((len(pay) + 3) // 4 + gaps[i % len(gaps)], FILL, np.int32)
        region.view(np.uint8)[:len(pay)] = pay
        desc.append((pos, frames + slack, frames, ch))
        words.append(region)
        pos += len(region)
    return np.concatenate(words), desc


def place_out(pcms, out, bits_out, **kw):
    """what the output buffer must hold in the end, and its descriptors"""
    if out == "wav":
        return place_wav(pcms, bits_out)
    return place(pcms, out, **kw)


def out_layout(hd, out, bits_out):
    return {16: hd.PCM_WAV16, 24: hd.PCM_WAV24}[bits_out] if out == "wav" else _layout(hd, out)


def poisoned(flat_want, desc, out, bits_out):
    """the output buffer before the call: the expected one with every stream's values replaced by other ones"""
    start = flat_want.copy()
    nb = bits_out // 8
    for off, stride, frames, ch in desc:
        if out == "wav":
            start.view(np.uint8)[4 * off:4 * off + frames * ch * nb] = 0x3C
        elif out == "planar":
            for c in range(ch):
                start[off + c * stride:off + c * stride + frames] = 0x3C3C3C3C
        else:
            start[off:off + frames * ch] = 0x3C3C3C3C
    return start


def run(hd, flat_in, layout_in, desc_in, start_out, out, desc_out, bits_in, bits_out, mode, frame0=None, **kw):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(flat_in).to(dev)
    d_out = torch.from_numpy(start_out).to(dev)
    got, d_rep = hd.pcm_requantize(d_in, _layout(hd, layout_in), desc_in, bits_in, bits_out, mode, SEED, frame0=frame0,
                                   out=d_out, layout_out=out_layout(hd, out, bits_out), desc_out=desc_out, **kw)
    assert got is d_out
    reports = hd.requant_list(d_rep)
    assert np.array_equal(d_in.cpu().numpy(), flat_in)           # the input is read only
    return d_out.cpu().numpy(), reports


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits_in,bits_out", DEPTHS)
@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("layout_in", LAYOUTS)
def test_sweep(pkg, layout_in, out, bits_in, bits_out, mode):
    """every channel count and length in one call; input and output off at each of the four dword alignments, each on
    its own cycle; planar strides odd; frame0 at every phase of the noise word's quad and far out"""
    hd = pkg.hipdec
    if out == "wav" and bits_out == 20:
        import torch
        for layout_out in (hd.PCM_WAV16, hd.PCM_WAV24):         # no payload has 20 bits
            with pytest.raises(hd.HipError, match="EINVAL"):
                hd.pcm_requantize(torch.zeros(64, dtype=torch.int32, device="cuda:0"), _layout(hd, layout_in), [(0, 8, 8, 1)],
                                  bits_in, bits_out, mode, layout_out=layout_out)
        return
    pcms = [sweep_pcm(ch, f, bits_in) for ch, f in SHAPES]
    frame0 = [FRAME0[i % len(FRAME0)] for i in range(len(SHAPES))]
    slack_in = [37 + (f & 1) for _, f in SHAPES] if layout_in == "planar" else [37]
    flat_in, desc_in = place(pcms, layout_in, slack_in, off_mod=[0, 1, 2, 3, 3, 2, 1])
    assert {d[0] % 4 for d in desc_in} == {0, 1, 2, 3}
    want = [want_of(ch, f, bits_in, bits_out, mode, frame0[i]) for i, (ch, f) in enumerate(SHAPES)]
    slack_out = [11 + (f & 1) for _, f in SHAPES] if out == "planar" else [9]
    flat_want, desc_out = place_out([w for w, _ in want], out, bits_out, slack=slack_out, off_mod=[2, 0, 3, 1, 1])
    if out == "planar":
        assert all(d[1] & 1 for d in desc_in if layout_in == "planar") and all(d[1] & 1 for d in desc_out)
    if out != "wav":
        assert len({(a[0] % 4, b[0] % 4) for a, b in zip(desc_in, desc_out)}) == 16
    got, reports = run(hd, flat_in, layout_in, desc_in, poisoned(flat_want, desc_out, out, bits_out), out, desc_out, bits_in,
                       bits_out, mode, frame0)
    for i, (ch, f) in enumerate(SHAPES):
        assert reports[i] == rm.report(f, want[i][1]), (i, ch, f, frame0[i])
    bad = np.flatnonzero(got != flat_want)
    assert bad.size == 0, (bad[:8], desc_out[:3])
    clipped = sum(sum(r["clipped"]) for r in reports)
    assert 0 < clipped < sum(ch * f for ch, f in SHAPES) * 3 // 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_aligned_streams_take_the_wide_path_to_the_same_values(pkg, layout):
    """16-byte aligned regions, strides multiples of 4, frame0 a multiple of 4: 16-byte accesses and one hash per quad
    and channel; with frame0 + 2 the same input gives the model's other values"""
    hd = pkg.hipdec
    shapes = [(2, 3 * T + 5), (6, T + 1024), (8, 2048), (1, 1027)]
    pcms = [sweep_pcm(ch, f, 24) for ch, f in shapes]
    for out, bits_out in (("planar", 16), ("interleaved", 20), ("wav", 16), ("wav", 24)):
        for base in (0, 2, 2 ** 40 - 4):
            frame0 = [base + 4 * i for i in range(len(shapes))]
            flat_in, desc_in = place(pcms, layout, [4 - f % 4 for _, f in shapes], off_mod=[0])
            want = [rm.requant_np(p, 24, bits_out, rm.TPDF, SEED, f0) for p, f0 in zip(pcms, frame0)]
            flat_want, desc_out = place_out([w for w, _ in want], out, bits_out, slack=[8 - f % 4 for _, f in shapes],
                                            off_mod=[0])
            assert all(d[0] % 4 == 0 and d[1] % 4 == 0 for d in desc_in)
            got, reports = run(hd, flat_in, layout, desc_in, poisoned(flat_want, desc_out, out, bits_out), out, desc_out, 24,
                               bits_out, rm.TPDF, frame0)
            assert np.array_equal(got, flat_want), (out, base)
            assert reports == [rm.report(p.shape[1], cl) for p, (_, cl) in zip(pcms, want)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_in_place_is_out_of_place(pkg, layout):
    import torch
    hd = pkg.hipdec
    pcms = [sweep_pcm(ch, f, 24) for ch, f in SHAPES]
    slack = [37 + (f & 1) for _, f in SHAPES] if layout == "planar" else [37]
    for off_mod in ([0, 1, 2, 3, 3, 2, 1], [0]):
        flat, desc = place(pcms, layout, slack if len(off_mod) > 1 else [8 - f % 4 for _, f in SHAPES], off_mod=off_mod)
        frame0 = [FRAME0[i % len(FRAME0)] for i in range(len(SHAPES))]
        d_in = torch.from_numpy(flat).to("cuda:0")
        d_other, d_rep = hd.pcm_requantize(d_in, _layout(hd, layout), desc, 24, 16, rm.TPDF, SEED, frame0=frame0)
        assert d_other.data_ptr() != d_in.data_ptr() and np.array_equal(d_in.cpu().numpy(), flat)
        d_same, d_rep2 = hd.pcm_requantize(d_in, _layout(hd, layout), desc, 24, 16, rm.TPDF, SEED, frame0=frame0, out=d_in)
        assert d_same is d_in
        assert np.array_equal(d_in.cpu().numpy(), d_other.cpu().numpy())
        assert hd.requant_list(d_rep) == hd.requant_list(d_rep2)
        want = [want_of(ch, f, 24, 16, rm.TPDF, frame0[i]) for i, (ch, f) in enumerate(SHAPES)]
        assert np.array_equal(d_in.cpu().numpy(), place([w for w, _ in want], layout, slack if len(off_mod) > 1 else
                                                        [8 - f % 4 for _, f in SHAPES], off_mod=off_mod)[0])


@pytest.mark.parametrize("bits", [16, 24])
def test_wav_output_is_pack_wav_of_the_int32_output(pkg, bits):
    hd = pkg.hipdec
    shapes = [(1, 65), (2, T + 1), (6, 3 * T + 5), (3, 1023)]       # (the packing kernel takes up to 6 channels)
    pcms = [sweep_pcm(ch, f, 24) for ch, f in shapes]
    flat_in, desc_in = place(pcms, "planar", [3], off_mod=[1, 0])
    zeros = [np.zeros_like(p) for p in pcms]
    start_p, desc_p = place(zeros, "planar", [0])
    start_w, desc_w = place_wav(zeros, bits)
    got_p, rep_p = run(hd, flat_in, "planar", desc_in, start_p, "planar", desc_p, 24, bits, rm.TPDF)
    got_w, rep_w = run(hd, flat_in, "planar", desc_in, start_w, "wav", desc_w, 24, bits, rm.TPDF)
    assert rep_p == rep_w
    for (off, stride, frames, ch), (woff, _, _, _) in zip(desc_p, desc_w):
        planar = got_p[off:off + ch * stride].reshape(ch, stride)[:, :frames]
        packed = hd.pack_wav(planar, bits)
        assert np.array_equal(got_w.view(np.uint8)[4 * woff:4 * woff + len(packed)], packed)
        assert len(packed) == frames * ch * bits // 8


@pytest.mark.parametrize("bits", [16, 20, 24])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pure_clamp_counts_what_the_level_report_calls_over(pkg, layout, bits):
    import torch
    hd = pkg.hipdec
    shapes = [(2, T + 1), (6, 777), (8, 2 * T)]
    pcms = [sweep_pcm(ch, f, bits) for ch, f in shapes]
    flat, desc = place(pcms, layout, [5], off_mod=[3, 0])
    d_in = torch.from_numpy(flat).to("cuda:0")
    levels = hd.levels_list(hd.pcm_levels(d_in, _layout(hd, layout), bits, desc))
    for mode in MODES:
        d_out, d_rep = hd.pcm_requantize(d_in, _layout(hd, layout), desc, bits, bits, mode, SEED)
        reports = hd.requant_list(d_rep)
        for p, lv, rep in zip(pcms, levels, reports):
            assert rep == rm.report(p.shape[1], lv["over"]) == rm.report(p.shape[1], lm.levels(p, bits)["over"])
            assert sum(rep["clipped"]) > 0
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        assert np.array_equal(d_out.cpu().numpy(), place([np.clip(p, lo, hi) for p in pcms], layout, [5], off_mod=[3, 0])[0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dirtied_workspaces_give_the_same_report(pkg, layout):
    """canaries around the workspace; its words 0xFF.. in one run, 0 in the other"""
    import torch
    hd = pkg.hipdec
    L = hd.lib()
    dev = torch.device("cuda", 0)
    shapes = [(3, 5 * T + 9), (8, T), (1, 1), (6, 2 * T + 1)]
    pcms = [sweep_pcm(ch, f, 24) for ch, f in shapes]
    flat, desc = place(pcms, layout, [3], off_mod=[1, 2])
    n, total = len(desc), sum(f for _, f in shapes)
    words = hd.pcm_requantize_workspace_words(n, total)
    d_in = torch.from_numpy(flat).to(dev)
    d_desc = torch.from_numpy(hd._desc_records(desc).view(np.uint8).reshape(-1)).to(dev)
    par = hd.Requant(24, 16, rm.TPDF, 0, SEED)
    results = []
    for fill in (-1, 0):
        d_out = torch.from_numpy(flat).to(dev)
        d_rep = torch.full((n * 72 + 16,), 0xEE, dtype=torch.uint8, device=dev)
        d_work = torch.full((words + 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_work[16:16 + words] = fill
        rc = L.dvda_pcm_hip_requantize(d_in.data_ptr(), _layout(hd, layout), d_desc.data_ptr(), d_out.data_ptr(),
                                       _layout(hd, layout), d_desc.data_ptr(), None, n, ctypes.byref(par), total,
                                       d_rep.data_ptr(), d_work.data_ptr() + 64, words,
                                       torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        work = d_work.cpu().numpy()
        assert (work[:16] == 0x5A5A5A5A).all() and (work[16 + words:] == 0x5A5A5A5A).all()
        rep = d_rep.cpu().numpy()
        assert (rep[n * 72:] == 0xEE).all()
        results.append((hd.requant_list(d_rep[:n * 72].reshape(n, 72)), d_out.cpu().numpy()))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
    want = [rm.requant_np(p, 24, 16, rm.TPDF, SEED, 0) for p in pcms]
    assert results[0][0] == [rm.report(p.shape[1], cl) for p, (_, cl) in zip(pcms, want)]
    assert np.array_equal(results[0][1], place([w for w, _ in want], layout, [3], off_mod=[1, 2])[0])


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_three_pieces_are_the_whole(pkg, layout, out):
    """a stream cut at frames that are no multiple of 4 or of the tile, each piece a call of its own with its frame0"""
    hd = pkg.hipdec
    ch, frames, start = 6, 3 * T + 5, 2 ** 33 + 3
    whole = sweep_pcm(ch, frames, 24)
    cuts = [0, 1001, T + 2050, frames]
    flat_in, desc_in = place([whole], layout, [2], off_mod=[1])
    want, cl = want_of(ch, frames, 24, 16, rm.TPDF, start)
    flat_want, desc_out = place_out([want], out, 16, slack=[7], off_mod=[2])
    got_whole, rep_whole = run(hd, flat_in, layout, desc_in, poisoned(flat_want, desc_out, out, 16), out, desc_out, 24, 16,
                               rm.TPDF, [start])
    assert np.array_equal(got_whole, flat_want) and rep_whole == [rm.report(frames, cl)]
    total = rm.report(0, [0] * 8)
    pieces = []
    for a, b in zip(cuts, cuts[1:]):
        part = np.ascontiguousarray(whole[:, a:b])
        flat_p, desc_p = place([part], layout, [1], off_mod=[3])
        want_p = np.ascontiguousarray(want[:, a:b])
        flat_wp, desc_op = place_out([want_p], out, 16, slack=[3], off_mod=[0])
        got_p, (rep,) = run(hd, flat_p, layout, desc_p, poisoned(flat_wp, desc_op, out, 16), out, desc_op, 24, 16, rm.TPDF,
                            [start + a])
        assert np.array_equal(got_p, flat_wp), (a, b)
        total = rm.report(total["frames"] + rep["frames"], [x + y for x, y in zip(total["clipped"], rep["clipped"])])
        pieces.append(rep)
    assert total == rep_whole[0] and sum(pieces[0]["clipped"]) and sum(pieces[1]["clipped"])


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_descriptors_that_are_not_taken_write_nothing(pkg, layout, out):
    hd = pkg.hipdec
    shapes = [(2, 100), (3, T + 7), (6, 50), (1, 9), (8, 300), (4, 64)]
    pcms = [sweep_pcm(ch, f, 24) for ch, f in shapes]
    flat_in, desc_in = place(pcms, layout, [3], off_mod=[0, 1])
    want = [rm.requant_np(p, 24, 16, rm.ROUND) for p in pcms]
    flat_want, desc_out = place_out([w for w, _ in want], out, 16, slack=[4], off_mod=[1])
    start = poisoned(flat_want, desc_out, out, 16)
    # 0 channels, 9 channels, an output stride below the frames, other frames, other channels: each on one stream
    desc_in[0] = desc_in[0][:3] + (0,)
    desc_in[1] = desc_in[1][:3] + (9,)
    desc_out[2] = (desc_out[2][0], desc_out[2][2] - 1) + desc_out[2][2:]
    desc_out[3] = desc_out[3][:2] + (desc_out[3][2] - 1, desc_out[3][3])
    desc_out[4] = desc_out[4][:3] + (7,)
    got, reports = run(hd, flat_in, layout, desc_in, start, out, desc_out, 24, 16, rm.ROUND)
    assert reports[:5] == [rm.report(0, [0] * 8)] * 5 and reports[5] == rm.report(64, want[5][1])
    expect = start.copy()
    off, stride, frames, ch = desc_out[5]
    lo, hi = (off, off + (frames * ch * 2 + 3) // 4) if out == "wav" else (off, off + stride * ch)
    expect[lo:hi] = flat_want[lo:hi]
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_bound_that_cuts_the_list(pkg, layout):
    """streams whose tiles lie inside max_total_frames are done; the one the bound cuts reports zeros and nothing outside
    its region changes; the ones behind it are untouched"""
    hd = pkg.hipdec
    shapes = [(2, T + 1), (3, 2 * T), (6, 3 * T + 5), (1, 100), (8, 10)]
    pcms = [sweep_pcm(ch, f, 24) for ch, f in shapes]
    n = len(shapes)
    flat, desc = place(pcms, layout, [6], off_mod=[2, 1])
    tiles = [-(-f // T) for _, f in shapes]
    bound = 1 * T               # max_tiles = bound / T + n = 6: streams 0 and 1 whole (4 tiles), 2 of stream 2's four
    assert tiles[0] + tiles[1] < bound // T + n < sum(tiles[:3])
    want = [rm.requant_np(p, 24, 16, rm.TPDF, SEED) for p in pcms]
    flat_want = place([w for w, _ in want], layout, [6], off_mod=[2, 1])[0]
    got, reports = run(hd, flat, layout, desc, flat.copy(), layout, desc, 24, 16, rm.TPDF, max_total_frames=bound)
    assert reports[:2] == [rm.report(p.shape[1], cl) for p, (_, cl) in zip(pcms[:2], want[:2])]
    assert reports[2:] == [rm.report(0, [0] * 8)] * 3
    lo = desc[2][0]
    hi = lo + desc[2][1] * desc[2][3]
    assert np.array_equal(got[:lo], flat_want[:lo]) and np.array_equal(got[hi:], flat[hi:])
    # inside the cut stream's region: only its own elements may have changed
    region, before = got[lo:hi], flat[lo:hi]
    if layout == "planar":
        region, before = region.reshape(desc[2][3], desc[2][1]), before.reshape(desc[2][3], desc[2][1])
        assert np.array_equal(region[:, desc[2][2]:], before[:, desc[2][2]:])
    else:
        assert np.array_equal(region[desc[2][2] * desc[2][3]:], before[desc[2][2] * desc[2][3]:])


# ---- behind a decode
def synth_stream(pkg, channels, bits, seed):
    """the small synthetic titles of the presentation tests (tests/test_presentation_model.make_stream), at either depth"""
    syn = pkg.synth
    kw = dict(assignment=12, n_substreams=2, ss0_channels=2) if channels == 6 else dict(assignment=1, n_substreams=1)
    cfg = syn.make_cfg(rate_code=1, n_aus=48, restart_interval=8, bps_code={16: 0, 20: 1, 24: 2}[bits], **kw)
    return syn.stream(cfg, 7000 + 13 * seed)[0]


_DECODED = {}


def decoded(pkg, layout):
    """four titles -- 2 and 6 channels, 24 and 16 bits -- and what decode_streams gives for them; decoded once"""
    if layout not in _DECODED:
        hd = pkg.hipdec
        streams = [synth_stream(pkg, ch, bits, i) for i, (ch, bits) in enumerate([(2, 24), (6, 24), (2, 16), (6, 16)])]
        pcm, infos = hd.decode_streams(streams, layout=_layout(hd, layout))
        assert [int(i.channels) for i in infos] == [2, 6, 2, 6] and all(i.status & ~hd.ST_BENIGN == 0 for i in infos)
        assert [hd.BITS_OF_CODE[int(i.group0_bps)] for i in infos] == [24, 24, 16, 16]
        _DECODED[layout] = (streams, pcm)
    return _DECODED[layout]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_streams_requantized(pkg, layout, mode):
    hd = pkg.hipdec
    streams, plain = decoded(pkg, layout)
    depth = [24, 24, 16, 16]
    pcm, infos, reports = hd.decode_streams_requantized(streams, 16, mode, seed=5, layout=_layout(hd, layout))
    pay, _, reports_w = hd.decode_streams_requantized(streams, 16, mode, seed=5, layout=_layout(hd, layout), wav=True)
    for i, p in enumerate(plain):
        want, cl = rm.requant_np(p, depth[i], 16, mode, 5, 0)
        assert np.array_equal(pcm[i], want) and reports[i] == reports_w[i] == rm.report(p.shape[1], cl), i
        assert pay[i].tobytes() == rm.payload(want, 16), i
    assert not np.array_equal(pcm[0], plain[0]) and int(infos[1].pcm_frames) == plain[1].shape[1]
    # 20 bits: the 24-bit titles are reduced, the 16-bit ones come out as decoded
    pcm, infos, reports = hd.decode_streams_requantized(streams, 20, mode, seed=5, layout=_layout(hd, layout))
    for i, p in enumerate(plain):
        if depth[i] == 24:
            want, cl = rm.requant_np(p, 24, 20, mode, 5, 0)
            assert np.array_equal(pcm[i], want) and reports[i] == rm.report(p.shape[1], cl)
        else:
            assert np.array_equal(pcm[i], p) and reports[i] is None


def test_decode_streams_requantized_presentation_and_shapes(pkg):
    hd = pkg.hipdec
    streams, plain = decoded(pkg, "planar")
    two, infos2 = hd.decode_streams([streams[1]], presentation=hd.PRESENT_SUBSTREAM0)
    assert two[0].shape[0] == 2
    pcm, infos, reports = hd.decode_streams_requantized([streams[1]], 16, hd.RQ_ROUND, presentation=hd.PRESENT_SUBSTREAM0)
    want, cl = rm.requant_np(two[0], 24, 16, rm.ROUND)
    assert np.array_equal(pcm[0], want) and reports == [rm.report(want.shape[1], cl)] and int(infos[0].channels) == 2
    assert len(hd.decode_streams([streams[0]])) == 2            # decode_streams' own tuple is as it was
    for bad in (dict(layout=hd.PCM_WAV16), dict(bits_out=20, wav=True)):
        with pytest.raises(hd.HipError, match="EINVAL"):
            hd.decode_streams_requantized([streams[0]], **{"bits_out": 16, **bad})


@pytest.mark.parametrize("layout", LAYOUTS)
def test_context_in_place_then_the_other_reports(pkg, layout):
    """Context.pcm_requantize on the decode's buffers; behind it the digest at 16 bits is zlib's of the model's payload and
    the level report the model's of the requantized PCM; a WAV-layout context is EINVAL"""
    hd = pkg.hipdec
    streams, plain = decoded(pkg, layout)
    streams, plain = streams[:2], plain[:2]
    frame0 = [3, 2 ** 40 - 5]
    batch = hd.Batch(streams)
    st = batch.current_stream
    ctx = hd.Context(0, batch.n, max(64, batch.total // 64), layout=_layout(hd, layout))
    try:
        ctx.index_batch(batch, st)
        infos = ctx.stream_info(stream=st)
        out = hd.PcmRegions.for_infos(infos, _layout(hd, layout), 0)
        ctx.decode(*out.ptrs, st)
        infos = ctx.stream_info(stream=st)
        assert all(np.array_equal(a, b) for a, b in zip(out.to_host(infos), plain))
        reports = ctx.pcm_requantize(*out.ptrs, 24, 16, hd.RQ_TPDF, seed=77, frame0=frame0, stream=st)
        want = [rm.requant_np(p, 24, 16, rm.TPDF, 77, f0) for p, f0 in zip(plain, frame0)]
        assert reports == [rm.report(p.shape[1], cl) for p, (_, cl) in zip(plain, want)]
        assert all(np.array_equal(a, w) for a, (w, _) in zip(out.to_host(infos), want))
        digests = ctx.pcm_crc32(*out.ptrs, 16, stream=st)
        assert digests == [(zlib.crc32(rm.payload(w, 16)), w.size * 2) for w, _ in want]
        assert ctx.pcm_levels(*out.ptrs, 16, stream=st) == [lm.levels(w, 16) for w, _ in want]
        assert all(sum(lv["over"]) == 0 for lv in ctx.pcm_levels(*out.ptrs, 16, stream=st))
        # a second pass at the same depth is a pure clamp of values already in range: nothing changes, nothing clips
        again = ctx.pcm_requantize(*out.ptrs, 16, 16, hd.RQ_TPDF, stream=st)
        assert again == [rm.report(p.shape[1], [0] * 8) for p in plain]
        assert all(np.array_equal(a, w) for a, (w, _) in zip(out.to_host(infos), want))
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_requantize(*out.ptrs, 16, 24, stream=st)
        ctx.set_pcm_layout(hd.PCM_WAV16)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_requantize(*out.ptrs, 24, 16, stream=st)
    finally:
        ctx.close()


def test_overflowed_stream_is_untouched(pkg):
    """a stream given too small a capacity carries DVDA_ST_OVERFLOW: zeros reported, its region as the decode left it"""
    hd = pkg.hipdec
    streams, plain = decoded(pkg, "planar")
    streams, plain = streams[:2], plain[:2]
    batch = hd.Batch(streams)
    st = batch.current_stream
    ctx = hd.Context(0, batch.n, max(64, batch.total // 64))
    try:
        ctx.index_batch(batch, st)
        rows = [plain[0].shape[1] // 2, plain[1].shape[1]]
        out = hd.PcmRegions(rows, [2, 6], hd.PCM_PLANAR, 0)
        ctx.decode(*out.ptrs, st)
        infos = ctx.stream_info(stream=st)
        assert infos[0].status & hd.ST["OVERFLOW"] and not infos[1].status & hd.ST["OVERFLOW"]
        before = out.d_pcm.cpu().numpy().copy()
        reports = ctx.pcm_requantize(*out.ptrs, 24, 16, hd.RQ_ROUND, stream=st)
        want, cl = rm.requant_np(plain[1], 24, 16, rm.ROUND)
        assert reports == [rm.report(0, [0] * 8), rm.report(plain[1].shape[1], cl)]
        after = out.d_pcm.cpu().numpy()
        cut = out.out_off[1]
        assert np.array_equal(after[:cut], before[:cut])
        assert np.array_equal(after[cut:cut + 6 * rows[1]].reshape(6, rows[1]), want)
    finally:
        ctx.close()
