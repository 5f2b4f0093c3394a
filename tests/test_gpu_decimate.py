"""The decimation on the GPU (dvda_pcm_hip_decimate, dvda_mlp_hip_pcm_decimate; csrc/pcm_decim.h): what the device writes
and what it counts is tests/decimate_model of the same values; nothing else in the output buffer changes.  Every
comparison is exact."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import decimate_model as dm
from tests.test_gpu_levels import FILL, LAYOUTS, _layout, place

pytestmark = pytest.mark.gpu

T = dm.TILE
CHANNELS = [1, 2, 6, 8]
PAIRS = [(a, b) for a in LAYOUTS for b in LAYOUTS]
_TAPS, _PCM, _WANT = {}, {}, {}


def frames_of(D):
    H = dm.half(D)
    return [0, 1, D - 1, D, H, H + 1, 2 * H + 1, D * T - 1, D * T, D * T + 1, 2 * D * T + 3]


def shapes_of(D):
    return [(ch, f) for ch in CHANNELS for f in frames_of(D)]


def taps(hd, D):
    if D not in _TAPS:
        _TAPS[D] = [int(v) for v in hd.decim_taps(D)]
    return _TAPS[D]


def mixed_pcm(rng, ch, frames):
    """the full int32 range in the first quarter, then values inside 24 bits: some outputs clip, most do not"""
    pcm = rng.integers(-2 ** 31, 2 ** 31, (ch, frames), dtype=np.int64)
    a = frames // 4
    pcm[:, a:] = rng.integers(-2 ** 23, 2 ** 23, (ch, frames - a), dtype=np.int64)
    return pcm.astype(np.int32)


def sweep_pcm(ch, frames):
    """computed once, shared, never written to"""
    key = (ch, frames)
    if key not in _PCM:
        _PCM[key] = mixed_pcm(np.random.default_rng(1000 * ch + frames), ch, frames)
        _PCM[key].setflags(write=False)
    return _PCM[key]


def want_of(hd, ch, frames, D, bits):
    key = (ch, frames, D, bits)
    if key not in _WANT:
        out, cl = dm.decimate_np(sweep_pcm(ch, frames), taps(hd, D), D, bits)
        out.setflags(write=False)
        _WANT[key] = (out, cl)
    return _WANT[key]


def poisoned(flat_want, desc, layout):
    """the output buffer before the call: the expected one with every stream's values replaced by other ones"""
    start = flat_want.copy()
    for off, stride, frames, ch in desc:
        if layout == "planar":
            for c in range(ch):
                start[off + c * stride:off + c * stride + frames] = 0x3C3C3C3C
        else:
            start[off:off + frames * ch] = 0x3C3C3C3C
    return start


def run(hd, flat_in, layout_in, desc_in, start_out, layout_out, desc_out, D, bits, pieces=None, **kw):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(flat_in).to(dev)
    d_out = torch.from_numpy(start_out).to(dev)
    got, _, d_rep = hd.pcm_decimate(d_in, _layout(hd, layout_in), desc_in, D, bits, pieces=pieces, out=d_out,
                                    layout_out=_layout(hd, layout_out), desc_out=desc_out, **kw)
    assert got is d_out
    reports = hd.decim_list(d_rep)
    assert np.array_equal(d_in.cpu().numpy(), flat_in)           # the input is read only
    return d_out.cpu().numpy(), reports


def check(hd, pcms, want, layout_in, layout_out, D, bits, slack_in, slack_out, off_in, off_out, pieces=None, frames_in=None):
    """places the inputs and the expected outputs, runs, compares the whole output buffer and the reports"""
    flat_in, desc_in = place(pcms, layout_in, slack_in, off_mod=off_in)
    flat_want, desc_out = place([w for w, _ in want], layout_out, slack_out, off_mod=off_out)
    got, reports = run(hd, flat_in, layout_in, desc_in, poisoned(flat_want, desc_out, layout_out), layout_out, desc_out, D,
                       bits, pieces)
    own = frames_in if frames_in is not None else [p.shape[1] for p in pcms]
    for i, (w, cl) in enumerate(want):
        assert reports[i] == dm.report(own[i], w.shape[1], cl), (i, pcms[i].shape)
    bad = np.flatnonzero(got != flat_want)
    assert bad.size == 0, (bad[:8], desc_out[:3])
    return reports, desc_in, desc_out


@pytest.mark.parametrize("layout_in,layout_out", PAIRS)
@pytest.mark.parametrize("D", dm.RATIOS)
def test_sweep(pkg, D, layout_in, layout_out):
    """every channel count and length in one call: every seam and every ragged end of the tile list; input and output off
    at each of the four dword alignments, each on its own cycle; planar strides of either parity"""
    hd = pkg.hipdec
    shapes = shapes_of(D)
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    want = [want_of(hd, ch, f, D, 24) for ch, f in shapes]
    assert [w.shape[1] for w, _ in want] == [-(-f // D) for _, f in shapes]
    slack_in = [37 + (f & 1) for _, f in shapes] if layout_in == "planar" else [37]
    slack_out = [11 + (-(-f // D) & 1) for _, f in shapes] if layout_out == "planar" else [9]
    reports, desc_in, desc_out = check(hd, pcms, want, layout_in, layout_out, D, 24, slack_in, slack_out,
                                       [0, 1, 2, 3, 3, 2, 1], [2, 0, 3, 1, 1])
    assert {d[0] % 4 for d in desc_in} == {0, 1, 2, 3} and {d[0] % 4 for d in desc_out} == {0, 1, 2, 3}
    assert len({(a[0] % 4, b[0] % 4) for a, b in zip(desc_in, desc_out)}) == 16
    clipped = sum(sum(r["clipped"]) for r in reports)
    assert 0 < clipped < sum(ch * w.shape[1] for (ch, _), (w, _) in zip(shapes, want)) // 2


@pytest.mark.parametrize("bits", dm.DEPTHS)
@pytest.mark.parametrize("D", dm.RATIOS)
def test_rails_overshoot_and_are_counted(pkg, D, bits):
    """full-scale square waves of several periods: the band-limited version overshoots, the clamp holds it and counts it"""
    hd = pkg.hipdec
    hi = (1 << (bits - 1)) - 1
    pcms = []
    for ch, frames in ((2, D * T + 77), (6, 3000), (8, 2 * D * T + 3)):
        idx = np.arange(frames)
        pcms.append(np.stack([np.where((idx // (5 + 3 * c + D)) % 2, hi, -hi - 1) for c in range(ch)]).astype(np.int32))
    want = [dm.decimate_np(p, taps(hd, D), D, bits) for p in pcms]
    assert all(cl[c] > 0 for p, (_, cl) in zip(pcms, want) for c in range(p.shape[0]))
    assert all(w.max() == hi and w.min() == -hi - 1 for w, _ in want)
    for layout_in, layout_out in (("planar", "interleaved"), ("interleaved", "planar")):
        check(hd, pcms, want, layout_in, layout_out, D, bits, [3], [2], [1, 2], [3, 0])


def impulse_positions(D, frames):
    """the first frames, the last frames, and +-H (and its neighbours) around each seam of the tile list"""
    H = dm.half(D)
    pos = [0, 1, D - 1, D, D + 1, frames - 1, frames - 2, frames - D, frames - D - 1]
    for seam in range(D * T, frames, D * T):
        pos += [seam - H - 1, seam - H, seam - H + 1, seam - 1, seam, seam + 1, seam + H - 1, seam + H, seam + H + 1]
    return [p for p in pos if 0 <= p < frames]


@pytest.mark.parametrize("layout_in,layout_out", PAIRS)
@pytest.mark.parametrize("D", dm.RATIOS)
def test_an_impulse_reads_the_table_back(pkg, D, layout_in, layout_out):
    """one impulse of 2^20 per channel: output M is tap H + D M - position, rounded once -- at the track's ends and on
    both sides of every seam of the tile list"""
    hd = pkg.hipdec
    t, H = taps(hd, D), dm.half(D)
    frames = 2 * D * T + 3
    pos = impulse_positions(D, frames)
    pcms, want = [], []
    for k in range(0, len(pos), 8):
        group = pos[k:k + 8]
        p = np.zeros((len(group), frames), np.int32)
        w = np.zeros((len(group), -(-frames // D)), np.int32)
        for c, at in enumerate(group):
            p[c, at] = 1 << 20
            for m in range(w.shape[1]):
                j = H + at - D * m                  # the tap that meets the impulse
                if 0 <= j < len(t):
                    w[c, m] = (t[j] * (1 << 20) + (1 << 29)) >> 30
        assert np.array_equal(w, dm.decimate_np(p, t, D, 24)[0])
        pcms.append(p)
        want.append((w, [0] * 8))
    check(hd, pcms, want, layout_in, layout_out, D, 24, [5], [3], [3, 1], [1, 2])


@pytest.mark.parametrize("D", dm.RATIOS)
def test_a_constant_comes_back_exactly(pkg, D):
    """exact v wherever the window lies inside the track (the gain at DC is exactly 1), the taper at both ends as the
    model has it"""
    hd = pkg.hipdec
    H = dm.half(D)
    values = [1, -1, 2 ** 23 - 1, -2 ** 23, 123456, -7654321]
    frames = D * T + 2 * H + 9
    p = np.stack([np.full(frames, v, np.int32) for v in values])
    w, cl = dm.decimate_np(p, taps(hd, D), D, 24)
    inside = [m for m in range(w.shape[1]) if D * m - H >= 0 and D * m + H < frames]
    assert len(inside) > T and all((w[c, inside] == v).all() for c, v in enumerate(values))
    assert not (w[2, :H // D] == values[2]).all()
    for layout in LAYOUTS:
        check(hd, [p], [(w, cl)], layout, layout, D, 24, [1], [1], [1], [3])


@pytest.mark.parametrize("layout_in,layout_out", PAIRS)
@pytest.mark.parametrize("D", dm.RATIOS)
def test_aligned_streams_take_the_wide_path_to_the_same_values(pkg, D, layout_in, layout_out):
    """16-byte aligned regions with strides that are multiples of 4: 16-byte loads and stores, the values of the sweep"""
    hd = pkg.hipdec
    shapes = [(2, 2 * D * T + 3), (6, D * T + 1), (8, D * T), (1, 2 * dm.half(D) + 1)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    want = [want_of(hd, ch, f, D, 24) for ch, f in shapes]
    reports, desc_in, desc_out = check(hd, pcms, want, layout_in, layout_out, D, 24, [4 - f % 4 for _, f in shapes],
                                       [8 - (-(-f // D)) % 4 for _, f in shapes], [0], [0])
    assert all(d[0] % 4 == 0 and d[1] % 4 == 0 for d in desc_in + desc_out)


@pytest.mark.parametrize("layout_in,layout_out", [("planar", "planar"), ("interleaved", "interleaved"), ("planar", "interleaved")])
@pytest.mark.parametrize("D", dm.RATIOS)
def test_three_pieces_are_the_whole(pkg, D, layout_in, layout_out):
    """a track cut at frames that are no multiple of D; context exactly H, longer than H, and cut short by the track's
    ends: all nine pieces in one call, each triple concatenated is the whole and its reports add up.  A piece with less
    than H of context differs from the whole exactly as the model with zeros says."""
    hd = pkg.hipdec
    t, H = taps(hd, D), dm.half(D)
    ch, frames = 6, 2 * D * T + 1001
    track = sweep_pcm(ch, frames)
    whole, cw = want_of(hd, ch, frames, D, 24)
    cuts = [0, 1001, D * T + 2051, frames]
    assert all(c % 2 for c in cuts[1:])
    regions, pieces, want, own = [], [], [], []
    for context in (H, H + 77, 10 ** 6):
        for a, b in zip(cuts, cuts[1:]):
            region, frame0, before, after = dm.cut(track, a, b, context, context)
            regions.append(np.ascontiguousarray(region))
            pieces.append((frame0, before, after))
            m0 = -(-a // D)
            nm = dm.out_frames(a, b - a, D)
            want.append((np.ascontiguousarray(whole[:, m0:m0 + nm]), dm.decimate_np(region, t, D, 24, frame0, before, after)[1]))
            own.append(b - a)
    reports, _, _ = check(hd, regions, want, layout_in, layout_out, D, 24, [3], [2], [1, 2, 3], [2, 3], pieces, own)
    for k in range(0, 9, 3):
        total = dm.report(0, 0, [0] * 8)
        for r in reports[k:k + 3]:
            total = dm.add_reports(total, r)
        assert total == dm.report(frames, whole.shape[1], cw) and sum(cw) > 0
        assert sum(w.shape[1] for w, _ in want[k:k + 3]) == whole.shape[1]
    # too little context: another signal, the model's with zeros where the context was cut
    region, frame0, before, after = dm.cut(track, cuts[1], cuts[2], H // 2, H // 2)
    short = dm.decimate_np(region, t, D, 24, frame0, before, after)
    m0 = -(-cuts[1] // D)
    assert not np.array_equal(short[0], whole[:, m0:m0 + short[0].shape[1]])
    check(hd, [np.ascontiguousarray(region)], [short], layout_in, layout_out, D, 24, [1], [1], [3], [1],
          [(frame0, before, after)], [cuts[2] - cuts[1]])


@pytest.mark.parametrize("layout_in,layout_out", [("planar", "planar"), ("interleaved", "interleaved")])
@pytest.mark.parametrize("D", dm.RATIOS)
def test_streams_that_are_not_taken_write_nothing(pkg, D, layout_in, layout_out):
    hd = pkg.hipdec
    shapes = [(2, 100), (3, D * T + 7), (6, 50), (1, 9), (8, 300), (4, 64), (2, 500), (2, 640)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    want = [dm.decimate_np(p, taps(hd, D), D, 24) for p in pcms]
    flat_in, desc_in = place(pcms, layout_in, [3], off_mod=[0, 1])
    flat_want, desc_out = place([w for w, _ in want], layout_out, [4], off_mod=[1])
    start = poisoned(flat_want, desc_out, layout_out)
    pieces = [(0, 0, 0)] * len(shapes)
    # 0 channels, 9 channels, an output stride below the frames, other output frames (one too few), other channels, ...
    desc_in[0] = desc_in[0][:3] + (0,)
    desc_in[1] = desc_in[1][:3] + (9,)
    desc_out[2] = (desc_out[2][0], desc_out[2][2] - 1) + desc_out[2][2:]
    desc_out[3] = desc_out[3][:2] + (desc_out[3][2] - 1, desc_out[3][3])
    desc_out[4] = desc_out[4][:3] + (7,)
    # ... more context than frames, and -- stream 7 -- the input's own frame count as the output's
    pieces[6] = (0, 300, 201)
    desc_out[7] = desc_out[7][:2] + (640, 2)
    got, reports = run(hd, flat_in, layout_in, desc_in, start, layout_out, desc_out, D, 24, pieces)
    zero = dm.report(0, 0, [0] * 8)
    assert reports[:5] == [zero] * 5 and reports[6:] == [zero] * 2
    assert reports[5] == dm.report(64, want[5][0].shape[1], want[5][1])
    expect = start.copy()
    off, stride, frames, ch = desc_out[5]
    lo, hi = off, off + stride * ch
    expect[lo:hi] = flat_want[lo:hi]
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", dm.RATIOS)
def test_a_bound_that_cuts_the_list(pkg, D, layout):
    """streams whose tiles lie inside max_total_out_frames are done; the one the bound cuts reports zeros and nothing
    outside its region changes; the ones behind it are untouched"""
    hd = pkg.hipdec
    shapes = [(2, D * T + 1), (3, 2 * D * T), (6, 3 * D * T + 5), (1, 100), (8, 10)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    n = len(shapes)
    want = [dm.decimate_np(p, taps(hd, D), D, 24) for p in pcms]
    flat_in, desc_in = place(pcms, layout, [6], off_mod=[2, 1])
    flat_want, desc = place([w for w, _ in want], layout, [6], off_mod=[1, 3])
    tiles = [-(-w.shape[1] // T) for w, _ in want]
    bound = 1 * T               # max_tiles = bound / T + n = 6: streams 0 and 1 whole (4 tiles), 2 of stream 2's four
    assert tiles[0] + tiles[1] < bound // T + n < sum(tiles[:3])
    start = poisoned(flat_want, desc, layout)
    got, reports = run(hd, flat_in, layout, desc_in, start, layout, desc, D, 24, max_total_out_frames=bound)
    assert reports[:2] == [dm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(pcms[:2], want[:2])]
    assert reports[2:] == [dm.report(0, 0, [0] * 8)] * 3
    lo = desc[2][0]
    hi = lo + desc[2][1] * desc[2][3]
    assert np.array_equal(got[:lo], flat_want[:lo]) and np.array_equal(got[hi:], start[hi:])
    # inside the cut stream's region: only its own elements may have changed, the guard words are intact
    region, before = got[lo:hi], start[lo:hi]
    if layout == "planar":
        region, before = region.reshape(desc[2][3], desc[2][1]), before.reshape(desc[2][3], desc[2][1])
        assert np.array_equal(region[:, desc[2][2]:], before[:, desc[2][2]:])
    else:
        assert np.array_equal(region[desc[2][2] * desc[2][3]:], before[desc[2][2] * desc[2][3]:])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dirtied_workspaces_give_the_same_report(pkg, layout):
    """canaries around the workspace; its words 0xFF.. in one run, 0 in the other"""
    import torch
    hd = pkg.hipdec
    L = hd.lib()
    D = 2
    dev = torch.device("cuda", 0)
    shapes = [(3, 5 * T + 9), (8, D * T), (1, 1), (6, 2 * D * T + 1)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    want = [dm.decimate_np(p, taps(hd, D), D, 16) for p in pcms]
    flat, desc = place(pcms, layout, [3], off_mod=[1, 2])
    flat_want, desc_out = place([w for w, _ in want], layout, [3], off_mod=[3, 1])
    n, total = len(desc), sum(w.shape[1] for w, _ in want)
    words = hd.pcm_decimate_workspace_words(n, total)
    d_in = torch.from_numpy(flat).to(dev)
    d_desc = torch.from_numpy(hd._desc_records(desc).view(np.uint8).reshape(-1)).to(dev)
    d_desc_out = torch.from_numpy(hd._desc_records(desc_out).view(np.uint8).reshape(-1)).to(dev)
    results = []
    for fill in (-1, 0):
        d_out = torch.from_numpy(poisoned(flat_want, desc_out, layout)).to(dev)
        d_rep = torch.full((n * 80 + 16,), 0xEE, dtype=torch.uint8, device=dev)
        d_work = torch.full((words + 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_work[16:16 + words] = fill
        rc = L.dvda_pcm_hip_decimate(d_in.data_ptr(), _layout(hd, layout), d_desc.data_ptr(), d_out.data_ptr(),
                                     _layout(hd, layout), d_desc_out.data_ptr(), None, n, D, 16, total, d_rep.data_ptr(),
                                     d_work.data_ptr() + 64, words, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        work = d_work.cpu().numpy()
        assert (work[:16] == 0x5A5A5A5A).all() and (work[16 + words:] == 0x5A5A5A5A).all()
        rep = d_rep.cpu().numpy()
        assert (rep[n * 80:] == 0xEE).all()
        results.append((hd.decim_list(d_rep[:n * 80].reshape(n, 80)), d_out.cpu().numpy()))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
    assert results[0][0] == [dm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(pcms, want)]
    assert np.array_equal(results[0][1], flat_want)


# ---- behind a decode
def synth_stream(pkg, channels, bits, rate_code, seed):
    """small synthetic titles at 96 kHz (rate code 1) or 192 kHz (2)"""
    syn = pkg.synth
    kw = dict(assignment=12, n_substreams=2, ss0_channels=2) if channels == 6 else dict(assignment=1, n_substreams=1)
    cfg = syn.make_cfg(rate_code=rate_code, n_aus=40, restart_interval=8, bps_code={16: 0, 20: 1, 24: 2}[bits], **kw)
    return syn.stream(cfg, 9000 + 13 * seed)[0]


TITLES = [(2, 24, 1), (6, 24, 2), (2, 16, 2), (6, 16, 1)]      # channels, bits, rate code
_DECODED = {}


def titles(pkg, oracle):
    """four titles and the oracle's PCM of them; made once"""
    if "t" not in _DECODED:
        streams = [synth_stream(pkg, ch, bits, rc, i) for i, (ch, bits, rc) in enumerate(TITLES)]
        plain = []
        for s, (ch, _, rc) in zip(streams, TITLES):
            pcm, frames, _ = oracle.decode(s, ch, 40 * 160 + 64)
            assert frames == 40 * (80 if rc == 1 else 160)
            plain.append(pcm)
        _DECODED["t"] = (streams, plain)
    return _DECODED["t"]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_streams_decimated(pkg, oracle, layout):
    hd = pkg.hipdec
    streams, plain = titles(pkg, oracle)
    pcm, rates, infos, reports = hd.decode_streams_decimated(streams, 2, layout=_layout(hd, layout))
    assert rates == [48000, 96000, 96000, 48000]
    for i, (p, (_, bits, _)) in enumerate(zip(plain, TITLES)):
        want, cl = dm.decimate_np(p, taps(hd, 2), 2, bits)
        assert np.array_equal(pcm[i], want) and reports[i] == dm.report(p.shape[1], want.shape[1], cl), i
        assert int(infos[i].pcm_frames) == p.shape[1]
    # by 4: only the 192 kHz titles have a rate to go to
    with pytest.raises(ValueError):
        hd.decode_streams_decimated(streams, 4, layout=_layout(hd, layout))
    pcm, rates, infos, reports = hd.decode_streams_decimated(streams[1:3], 4, layout=_layout(hd, layout))
    assert rates == [48000, 48000]
    for i in (1, 2):
        want, cl = dm.decimate_np(plain[i], taps(hd, 4), 4, TITLES[i][1])
        assert np.array_equal(pcm[i - 1], want) and reports[i - 1] == dm.report(plain[i].shape[1], want.shape[1], cl)
    assert len(hd.decode_streams([streams[0]])) == 2            # decode_streams' own tuple is as it was
    for bad in (dict(layout=hd.PCM_WAV16), dict(ratio=3)):
        with pytest.raises(hd.HipError, match="EINVAL"):
            hd.decode_streams_decimated([streams[0]], **{"ratio": 2, **bad})


@pytest.mark.parametrize("layout", LAYOUTS)
def test_context_decimate_then_requantize_then_digest(pkg, oracle, layout):
    """Context.pcm_decimate from the decode's buffers into a second buffer; pcm_requantize -> pcm_crc32 on the result is
    zlib's digest of the model's payload; a WAV-layout context is EINVAL"""
    import torch
    hd = pkg.hipdec
    streams, plain = titles(pkg, oracle)
    streams, plain = streams[:2], plain[:2]
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
        want = [dm.decimate_np(p, taps(hd, 2), 2, 24) for p in plain]
        flat_want, desc = place([w for w, _ in want], layout, [3], off_mod=[1, 2])
        d_dst = torch.from_numpy(poisoned(flat_want, desc, layout)).to("cuda:0")
        reports = ctx.pcm_decimate(*out.ptrs, 2, 24, d_dst.data_ptr(), _layout(hd, layout), [d[0] for d in desc],
                                   [d[1] for d in desc], stream=st)
        assert reports == [dm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(plain, want)]
        assert np.array_equal(d_dst.cpu().numpy(), flat_want)
        assert all(np.array_equal(a, b) for a, b in zip(out.to_host(infos), plain))     # the decode's PCM is as it was
        # the decimated buffer is PCM like any other: down to 16 bits in place, then its digest
        from tests import requant_model as rm
        _, d_rep = hd.pcm_requantize(d_dst, _layout(hd, layout), desc, 24, 16, hd.RQ_TPDF, seed=3, out=d_dst)
        low = [rm.requant_np(w, 24, 16, rm.TPDF, 3, 0) for w, _ in want]
        assert hd.requant_list(d_rep) == [rm.report(w.shape[1], cl) for w, cl in low]
        d_crc, d_nb = hd.pcm_crc32(d_dst, _layout(hd, layout), 16, desc)
        assert hd.crc_list(d_crc, d_nb) == [(zlib.crc32(dm.payload(w, 16)), w.size * 2) for w, _ in low]
        for bad in (dict(ratio=3), dict(bits=18), dict(layout_dst=hd.PCM_WAV16)):
            kw = {"ratio": 2, "bits": 24, "layout_dst": _layout(hd, layout), **bad}
            with pytest.raises(hd.HipError, match="EINVAL"):
                ctx.pcm_decimate(*out.ptrs, kw["ratio"], kw["bits"], d_dst.data_ptr(), kw["layout_dst"], [d[0] for d in desc],
                                 [d[1] for d in desc], stream=st)
        ctx.set_pcm_layout(hd.PCM_WAV16)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_decimate(*out.ptrs, 2, 24, d_dst.data_ptr(), _layout(hd, layout), [d[0] for d in desc],
                             [d[1] for d in desc], stream=st)
    finally:
        ctx.close()


def test_overflowed_stream_is_untouched(pkg, oracle):
    """a stream given too small a capacity carries DVDA_ST_OVERFLOW: zeros reported, nothing written for it"""
    import torch
    hd = pkg.hipdec
    streams, plain = titles(pkg, oracle)
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
        want, cl = dm.decimate_np(plain[1], taps(hd, 4), 4, 24)
        room = [np.zeros((2, plain[0].shape[1] // 4), np.int32), want]
        flat_want, desc = place(room, "planar", [2], off_mod=[3])
        start = poisoned(flat_want, desc, "planar")
        expect = start.copy()
        lo, hi = desc[1][0], desc[1][0] + desc[1][1] * 6
        expect[lo:hi] = flat_want[lo:hi]
        d_dst = torch.from_numpy(start).to("cuda:0")
        reports = ctx.pcm_decimate(*out.ptrs, 4, 24, d_dst.data_ptr(), hd.PCM_PLANAR, [d[0] for d in desc],
                                   [d[1] for d in desc], stream=st)
        assert reports == [dm.report(0, 0, [0] * 8), dm.report(plain[1].shape[1], want.shape[1], cl)]
        assert np.array_equal(d_dst.cpu().numpy(), expect)
    finally:
        ctx.close()
