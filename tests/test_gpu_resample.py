"""The 48 kHz -> 44.1 kHz resampler on the GPU (dvda_pcm_hip_resample, dvda_mlp_hip_pcm_resample; csrc/pcm_resample.h):
what the device writes and what it counts is tests/resample_model of the same values; nothing else in the output buffer
changes.  Every comparison is exact."""
import numpy as np
import pytest

from tests import decimate_model as dm
from tests import resample_model as rm
from tests.test_gpu_levels import LAYOUTS, _layout, place

pytestmark = pytest.mark.gpu

T = rm.TILE
CHANNELS = [1, 2, 5, 6, 8]
PAIRS = [(a, b) for a in LAYOUTS for b in LAYOUTS]
_TABLE, _PCM, _WANT = {}, {}, {}


def frames_for(out):
    """the longest track that gives `out` output frames"""
    f = 160 * out // 147
    assert rm.out_frames(0, f) == out and rm.out_frames(0, f + 1) == out + 1
    return f


# every phase and both edges of the window; then the seams and ragged ends of the tile list
FRAMES = [0, 1, 47, 48, 49, 95, 96, 97, 159, 160, 161, 320] + [frames_for(o) for o in (T - 1, T, T + 1, 2 * T + 1)]
SHAPES = [(ch, f) for ch in CHANNELS for f in FRAMES]


def table(hd):
    if "t" not in _TABLE:
        _TABLE["t"] = hd.resample_taps()
    return _TABLE["t"]


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


def want_of(hd, ch, frames, bits):
    key = (ch, frames, bits)
    if key not in _WANT:
        out, cl = rm.resample_np(sweep_pcm(ch, frames), table(hd), bits)
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


def run(hd, flat_in, layout_in, desc_in, start_out, layout_out, desc_out, bits, pieces=None, **kw):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(flat_in).to(dev)
    d_out = torch.from_numpy(start_out).to(dev)
    got, _, d_rep = hd.pcm_resample(d_in, _layout(hd, layout_in), desc_in, bits, pieces=pieces, out=d_out,
                                    layout_out=_layout(hd, layout_out), desc_out=desc_out, **kw)
    assert got is d_out
    reports = hd.decim_list(d_rep)
    assert np.array_equal(d_in.cpu().numpy(), flat_in)           # the input is read only
    return d_out.cpu().numpy(), reports


def check(hd, pcms, want, layout_in, layout_out, bits, slack_in, slack_out, off_in, off_out, pieces=None, frames_in=None):
    """places the inputs and the expected outputs, runs, compares the whole output buffer and the reports"""
    flat_in, desc_in = place(pcms, layout_in, slack_in, off_mod=off_in)
    flat_want, desc_out = place([w for w, _ in want], layout_out, slack_out, off_mod=off_out)
    got, reports = run(hd, flat_in, layout_in, desc_in, poisoned(flat_want, desc_out, layout_out), layout_out, desc_out,
                       bits, pieces)
    own = frames_in if frames_in is not None else [p.shape[1] for p in pcms]
    for i, (w, cl) in enumerate(want):
        assert reports[i] == rm.report(own[i], w.shape[1], cl), (i, pcms[i].shape)
    bad = np.flatnonzero(got != flat_want)
    assert bad.size == 0, (bad[:8], desc_out[:3])
    return reports, desc_in, desc_out


def test_the_numpy_model_is_the_integer_model_on_the_sweep(pkg):
    """(CPU arithmetic, here because it vouches for the oracle of this file: the short streams of the sweep, every phase)"""
    hd = pkg.hipdec
    for ch, f in [(2, f) for f in FRAMES if f <= 320]:
        a, ca = rm.resample(sweep_pcm(ch, f), table(hd), 24)
        b, cb = want_of(hd, ch, f, 24)
        assert np.array_equal(a, b) and ca == cb


@pytest.mark.parametrize("layout_in,layout_out", PAIRS)
def test_sweep(pkg, layout_in, layout_out):
    """every channel count and length in one call: every phase, both edges of the window, every seam and every ragged end
    of the tile list; input and output off at each of the four dword alignments, each on its own cycle; planar strides of
    either parity"""
    hd = pkg.hipdec
    pcms = [sweep_pcm(ch, f) for ch, f in SHAPES]
    want = [want_of(hd, ch, f, 24) for ch, f in SHAPES]
    assert [w.shape[1] for w, _ in want] == [-(-147 * f // 160) for _, f in SHAPES]
    assert {w.shape[1] for w, _ in want} >= {0, 1, T - 1, T, T + 1, 2 * T + 1}
    slack_in = [37 + (f & 1) for _, f in SHAPES] if layout_in == "planar" else [37]
    slack_out = [11 + (w.shape[1] & 1) for w, _ in want] if layout_out == "planar" else [9]
    reports, desc_in, desc_out = check(hd, pcms, want, layout_in, layout_out, 24, slack_in, slack_out,
                                       [0, 1, 2, 3, 3, 2, 1], [2, 0, 3, 1, 1])
    assert {d[0] % 4 for d in desc_in} == {0, 1, 2, 3} and {d[0] % 4 for d in desc_out} == {0, 1, 2, 3}
    assert len({(a[0] % 4, b[0] % 4) for a, b in zip(desc_in, desc_out)}) == 16
    if layout_in == "planar":
        assert {d[1] & 1 for d in desc_in if d[3] > 1} == {1}           # odd planar strides
    if layout_out == "planar":
        assert {d[1] & 1 for d in desc_out if d[3] > 1} == {1}
    clipped = sum(sum(r["clipped"]) for r in reports)
    assert 0 < clipped < sum(ch * w.shape[1] for (ch, _), (w, _) in zip(SHAPES, want)) // 2


@pytest.mark.parametrize("bits", rm.DEPTHS)
def test_rails_overshoot_and_are_counted(pkg, bits):
    """full-scale square waves of several periods: the band-limited version overshoots, the clamp holds it and counts
    it; the model alone says so first"""
    hd = pkg.hipdec
    hi = (1 << (bits - 1)) - 1
    pcms = []
    for ch, frames in ((2, frames_for(T) + 77), (5, 3000), (8, 2000)):
        idx = np.arange(frames)
        pcms.append(np.stack([np.where((idx // (6 + 3 * c)) % 2, hi, -hi - 1) for c in range(ch)]).astype(np.int32))
    want = [rm.resample_np(p, table(hd), bits) for p in pcms]
    assert all(cl[c] > 0 for p, (_, cl) in zip(pcms, want) for c in range(p.shape[0]))
    assert all(w.max() == hi and w.min() == -hi - 1 for w, _ in want)
    for layout_in, layout_out in (("planar", "interleaved"), ("interleaved", "planar")):
        check(hd, pcms, want, layout_in, layout_out, bits, [3], [2], [1, 2], [3, 0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_full_range_int32_input(pkg, layout):
    """every value anywhere in int32, and the two constant rails of int32: the accumulator does not overflow"""
    hd = pkg.hipdec
    rng = np.random.default_rng(77)
    pcms = [rng.integers(-2 ** 31, 2 ** 31, (6, 1500), dtype=np.int64).astype(np.int32),
            np.stack([np.full(700, -2 ** 31, np.int64), np.full(700, 2 ** 31 - 1, np.int64)]).astype(np.int32)]
    # ... and the signs of one phase's taps: the largest accumulator there is
    g = table(hd)[73].astype(np.int64)
    worst = np.zeros((2, 400), np.int64)
    worst[0, 100:196] = np.where(g >= 0, 2 ** 31 - 1, -2 ** 31)
    worst[1, 100:196] = np.where(g >= 0, -2 ** 31, 2 ** 31 - 1)
    pcms.append(worst.astype(np.int32))
    want = [rm.resample_np(p, table(hd), 24) for p in pcms]
    assert all(sum(cl) > 0 for _, cl in want)
    check(hd, pcms, want, layout, layout, 24, [2], [3], [1, 3], [2, 1])


def test_an_impulse_reads_the_table_back(pkg):
    """one impulse of 2^20 per channel: output m is tap 47 + position - q(m) of phase p(m), rounded once -- at the
    track's ends and on both sides of a seam of the tile list"""
    hd = pkg.hipdec
    g = table(hd)
    frames = frames_for(T) + 300
    seam = 160 * T // 147
    pos = [0, 1, 46, 47, 48, frames - 1, frames - 48, frames - 49, seam - 49, seam - 48, seam - 1, seam, seam + 1, seam + 46,
           seam + 47, seam + 48]
    pcms, want = [], []
    for k in range(0, len(pos), 8):
        group = pos[k:k + 8]
        p = np.zeros((len(group), frames), np.int32)
        w = np.zeros((len(group), rm.out_frames(0, frames)), np.int32)
        for c, at in enumerate(group):
            p[c, at] = 1 << 20
            for m in range(w.shape[1]):
                q, ph = divmod(160 * m, 147)
                i = at - (q - 47)
                if 0 <= i < 96:
                    w[c, m] = (int(g[ph][i]) * (1 << 20) + (1 << 29)) >> 30
        assert np.array_equal(w, rm.resample_np(p, g, 24)[0])
        pcms.append(p)
        want.append((w, [0] * 8))
    check(hd, pcms, want, "planar", "interleaved", 24, [5], [3], [3, 1], [1, 2])
    check(hd, pcms, want, "interleaved", "planar", 24, [5], [3], [3, 1], [1, 2])


def test_a_constant_comes_back_exactly(pkg):
    """exact v wherever the window lies inside the track (every phase sums to 2^30), the taper at both ends as the model
    has it"""
    hd = pkg.hipdec
    values = [1, -1, 2 ** 23 - 1, -2 ** 23, 123456]
    frames = 1000
    p = np.stack([np.full(frames, v, np.int32) for v in values])
    w, cl = rm.resample_np(p, table(hd), 24)
    inside = [m for m in range(w.shape[1]) if 160 * m // 147 - 47 >= 0 and 160 * m // 147 + 48 < frames]
    assert len(inside) > 700 and all((w[c, inside] == v).all() for c, v in enumerate(values))
    assert not (w[2, :40] == values[2]).all()
    for layout in LAYOUTS:
        check(hd, [p], [(w, cl)], layout, layout, 24, [1], [1], [1], [3])


@pytest.mark.parametrize("layout_in,layout_out", [("planar", "planar"), ("interleaved", "interleaved"), ("planar", "interleaved")])
def test_three_pieces_are_the_whole(pkg, layout_in, layout_out):
    """a track cut at arbitrary frames; context exactly 48, longer, and cut short by the track's ends: all nine pieces
    in one call, each triple concatenated is the whole and its reports add up.  A piece with less context differs from
    the whole exactly as the model with zeros says."""
    hd = pkg.hipdec
    g = table(hd)
    ch, frames = 6, frames_for(T) + 3001
    track = sweep_pcm(ch, frames)
    whole, cw = want_of(hd, ch, frames, 24)
    cuts = [0, 1001, frames_for(T) + 1051, frames]
    regions, pieces, want, own = [], [], [], []
    for context in (48, 48 + 77, 10 ** 6):
        for a, b in zip(cuts, cuts[1:]):
            region, frame0, before, after = rm.cut(track, a, b, context, context)
            regions.append(np.ascontiguousarray(region))
            pieces.append((frame0, before, after))
            m0 = rm.first_out(a)
            nm = rm.out_frames(a, b - a)
            want.append((np.ascontiguousarray(whole[:, m0:m0 + nm]), rm.resample_np(region, g, 24, frame0, before, after)[1]))
            own.append(b - a)
    reports, _, _ = check(hd, regions, want, layout_in, layout_out, 24, [3], [2], [1, 2, 3], [2, 3], pieces, own)
    for k in range(0, 9, 3):
        total = rm.report(0, 0, [0] * 8)
        for r in reports[k:k + 3]:
            total = rm.add_reports(total, r)
        assert total == rm.report(frames, whole.shape[1], cw) and sum(cw) > 0
        assert sum(w.shape[1] for w, _ in want[k:k + 3]) == whole.shape[1]
    # too little context: another signal, the model's with zeros where the context was cut; 47 in front is enough, 47
    # behind is not
    for cb, ca, same in ((24, 24, False), (47, 48, True), (48, 47, False), (0, 0, False)):
        region, frame0, before, after = rm.cut(track, cuts[1], cuts[2], cb, ca)
        short = rm.resample_np(region, g, 24, frame0, before, after)
        m0 = rm.first_out(cuts[1])
        assert np.array_equal(short[0], whole[:, m0:m0 + short[0].shape[1]]) == same
        holed = np.array(track)
        holed[:, :cuts[1] - cb] = 0
        holed[:, cuts[2] + ca:] = 0
        assert np.array_equal(short[0], rm.resample_np(holed, g, 24)[0][:, m0:m0 + short[0].shape[1]])
        check(hd, [np.ascontiguousarray(region)], [short], layout_in, layout_out, 24, [1], [1], [3], [1],
              [(frame0, before, after)], [cuts[2] - cuts[1]])


def test_a_piece_far_into_a_track(pkg):
    """frame0 beyond 2^32 and beyond 2^61: the phase and the window follow the absolute frame"""
    hd = pkg.hipdec
    g = table(hd)
    piece = sweep_pcm(2, 500)
    for frame0 in (2 ** 32 + 12345, 2 ** 61 + 777, 2 ** 62):
        before, after = 48, 48
        want = rm.resample(np.asarray(piece), g, 24, frame0, before, after)
        assert want[0].shape[1] == rm.out_frames(frame0, 404)
        check(hd, [piece], [want], "planar", "planar", 24, [1], [1], [1], [2], [(frame0, before, after)], [404])


@pytest.mark.parametrize("layout_in,layout_out", [("planar", "planar"), ("interleaved", "interleaved")])
def test_streams_that_are_not_taken_write_nothing(pkg, layout_in, layout_out):
    hd = pkg.hipdec
    shapes = [(2, 100), (3, frames_for(T) + 7), (6, 50), (1, 9), (8, 300), (4, 64), (2, 500), (2, 640), (2, 320)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    want = [rm.resample_np(p, table(hd), 24) for p in pcms]
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
    # ... more context than frames, the input's own frame count as the output's, a frame0 above 2^62
    pieces[6] = (0, 300, 201)
    desc_out[7] = desc_out[7][:2] + (640, 2)
    pieces[8] = (2 ** 62 + 1, 0, 0)
    got, reports = run(hd, flat_in, layout_in, desc_in, start, layout_out, desc_out, 24, pieces)
    zero = rm.report(0, 0, [0] * 8)
    assert reports[:5] == [zero] * 5 and reports[6:] == [zero] * 3
    assert reports[5] == rm.report(64, want[5][0].shape[1], want[5][1])
    expect = start.copy()
    off, stride, frames, ch = desc_out[5]
    lo, hi = off, off + stride * ch
    expect[lo:hi] = flat_want[lo:hi]
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_bound_that_cuts_the_list(pkg, layout):
    """streams whose tiles lie inside max_total_out_frames are done; the one the bound cuts reports zeros and nothing
    outside its region changes; the ones behind it are untouched"""
    hd = pkg.hipdec
    shapes = [(2, frames_for(T) + 1), (3, frames_for(2 * T)), (6, frames_for(3 * T) + 5), (1, 100), (8, 10)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    n = len(shapes)
    want = [rm.resample_np(p, table(hd), 24) for p in pcms]
    flat_in, desc_in = place(pcms, layout, [6], off_mod=[2, 1])
    flat_want, desc = place([w for w, _ in want], layout, [6], off_mod=[1, 3])
    tiles = [-(-w.shape[1] // T) for w, _ in want]
    bound = 1 * T               # max_tiles = bound / T + n = 6: streams 0 and 1 whole (4 tiles), 2 of stream 2's four
    assert tiles[0] + tiles[1] < bound // T + n < sum(tiles[:3])
    start = poisoned(flat_want, desc, layout)
    got, reports = run(hd, flat_in, layout, desc_in, start, layout, desc, 24, max_total_out_frames=bound)
    assert reports[:2] == [rm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(pcms[:2], want[:2])]
    assert reports[2:] == [rm.report(0, 0, [0] * 8)] * 3
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
    dev = torch.device("cuda", 0)
    shapes = [(3, frames_for(T) + 9), (8, 3000), (1, 1), (6, frames_for(2 * T) + 1)]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    want = [rm.resample_np(p, table(hd), 16) for p in pcms]
    flat, desc = place(pcms, layout, [3], off_mod=[1, 2])
    flat_want, desc_out = place([w for w, _ in want], layout, [3], off_mod=[3, 1])
    n, total = len(desc), sum(w.shape[1] for w, _ in want)
    words = hd.pcm_resample_workspace_words(n, total)
    d_in = torch.from_numpy(flat).to(dev)
    d_desc = torch.from_numpy(hd._desc_records(desc).view(np.uint8).reshape(-1)).to(dev)
    d_desc_out = torch.from_numpy(hd._desc_records(desc_out).view(np.uint8).reshape(-1)).to(dev)
    results = []
    for fill in (-1, 0):
        d_out = torch.from_numpy(poisoned(flat_want, desc_out, layout)).to(dev)
        d_rep = torch.full((n * 80 + 16,), 0xEE, dtype=torch.uint8, device=dev)
        d_work = torch.full((words + 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_work[16:16 + words] = fill
        rc = L.dvda_pcm_hip_resample(d_in.data_ptr(), _layout(hd, layout), d_desc.data_ptr(), d_out.data_ptr(),
                                     _layout(hd, layout), d_desc_out.data_ptr(), None, n, 16, total, d_rep.data_ptr(),
                                     d_work.data_ptr() + 64, words, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        work = d_work.cpu().numpy()
        assert (work[:16] == 0x5A5A5A5A).all() and (work[16 + words:] == 0x5A5A5A5A).all()
        rep = d_rep.cpu().numpy()
        assert (rep[n * 80:] == 0xEE).all()
        results.append((hd.decim_list(d_rep[:n * 80].reshape(n, 80)), d_out.cpu().numpy()))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
    assert results[0][0] == [rm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(pcms, want)]
    assert sum(sum(cl) for _, cl in want) > 0
    assert np.array_equal(results[0][1], flat_want)


# ---- behind a decode
def synth_stream(pkg, channels, bits, rate_code, seed):
    """small synthetic titles at 48 kHz (rate code 0), 96 kHz (1), 192 kHz (2), 44.1 kHz (8) or 88.2 kHz (9)"""
    syn = pkg.synth
    kw = dict(assignment=12, n_substreams=2, ss0_channels=2) if channels == 6 else dict(assignment=1, n_substreams=1)
    cfg = syn.make_cfg(rate_code=rate_code, n_aus=40, restart_interval=8, bps_code={16: 0, 20: 1, 24: 2}[bits], **kw)
    return syn.stream(cfg, 9100 + 13 * seed)[0]


TITLES = [(2, 24, 0), (6, 24, 1), (2, 16, 1), (6, 16, 0), (2, 24, 2), (2, 24, 8), (2, 16, 9)]      # channels, bits, rate code
ROWS = {0: 40, 8: 40, 1: 80, 9: 80, 2: 160}
_DECODED = {}


def titles(pkg, oracle):
    """the titles and the oracle's PCM of them; made once"""
    if "t" not in _DECODED:
        streams = [synth_stream(pkg, ch, bits, rc, i) for i, (ch, bits, rc) in enumerate(TITLES)]
        plain = []
        for s, (ch, _, rc) in zip(streams, TITLES):
            pcm, frames, _ = oracle.decode(s, ch, 40 * 160 + 64)
            assert frames == 40 * ROWS[rc]
            plain.append(pcm)
        _DECODED["t"] = (streams, plain)
    return _DECODED["t"]


def composed(hd, pcm, bits, rate_code):
    """the composition of the two models a stream of that rate goes through -> (pcm, decimate report, resample report)"""
    D = {0: 1, 8: 1, 1: 2, 9: 2, 2: 4}[rate_code]
    rep_d = rep_r = None
    if D > 1:
        out, cl = dm.decimate_np(pcm, [int(v) for v in hd.decim_taps(D)], D, bits)
        rep_d = dm.report(pcm.shape[1], out.shape[1], cl)
        pcm = out
    if rate_code in (0, 1, 2):
        out, cl = rm.resample_np(pcm, table(hd), bits)
        rep_r = rm.report(pcm.shape[1], out.shape[1], cl)
        pcm = out
    return pcm, rep_d, rep_r


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_streams_resampled(pkg, oracle, layout):
    hd = pkg.hipdec
    streams, plain = titles(pkg, oracle)
    pcm, infos, reports = hd.decode_streams_resampled(streams, layout=_layout(hd, layout))
    for i, (p, (_, bits, rc)) in enumerate(zip(plain, TITLES)):
        want, rep_d, rep_r = composed(hd, p, bits, rc)
        assert np.array_equal(pcm[i], want), i
        assert reports[i] == dict(decimate=rep_d, resample=rep_r), i
        assert int(infos[i].pcm_frames) == p.shape[1]
    assert pcm[0].shape[1] == -(-147 * plain[0].shape[1] // 160) and np.array_equal(pcm[5], plain[5])
    pcm, _, _ = hd.decode_streams_resampled(streams[:1], rate=44100, layout=_layout(hd, layout))
    assert np.array_equal(pcm[0], composed(hd, plain[0], 24, 0)[0])
    for rate in (48000, 0, 22050, 88200):
        with pytest.raises(ValueError):
            hd.decode_streams_resampled(streams[:1], rate=rate)
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.decode_streams_resampled(streams[:1], layout=hd.PCM_WAV16)
    assert len(hd.decode_streams([streams[0]])) == 2            # decode_streams' own tuple is as it was


@pytest.mark.parametrize("layout", LAYOUTS)
def test_context_resample(pkg, oracle, layout):
    """Context.pcm_resample from the decode's buffers into a second buffer: 48 kHz titles, and a 96 kHz one taken as it
    is (the call does not ask for the rate); a WAV-layout context, a bad depth or layout is EINVAL"""
    import torch
    hd = pkg.hipdec
    streams, plain = titles(pkg, oracle)
    pick = [0, 3, 1]
    streams, plain = [streams[i] for i in pick], [plain[i] for i in pick]
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
        want = [rm.resample_np(p, table(hd), 24) for p in plain]
        flat_want, desc = place([w for w, _ in want], layout, [3], off_mod=[1, 2])
        d_dst = torch.from_numpy(poisoned(flat_want, desc, layout)).to("cuda:0")
        reports = ctx.pcm_resample(*out.ptrs, 24, d_dst.data_ptr(), _layout(hd, layout), [d[0] for d in desc],
                                   [d[1] for d in desc], stream=st)
        assert reports == [rm.report(p.shape[1], w.shape[1], cl) for p, (w, cl) in zip(plain, want)]
        assert np.array_equal(d_dst.cpu().numpy(), flat_want)
        assert all(np.array_equal(a, b) for a, b in zip(out.to_host(infos), plain))     # the decode's PCM is as it was
        for bad in (dict(bits=18), dict(layout_dst=hd.PCM_WAV16)):
            kw = {"bits": 24, "layout_dst": _layout(hd, layout), **bad}
            with pytest.raises(hd.HipError, match="EINVAL"):
                ctx.pcm_resample(*out.ptrs, kw["bits"], d_dst.data_ptr(), kw["layout_dst"], [d[0] for d in desc],
                                 [d[1] for d in desc], stream=st)
        ctx.set_pcm_layout(hd.PCM_WAV16)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_resample(*out.ptrs, 24, d_dst.data_ptr(), _layout(hd, layout), [d[0] for d in desc],
                             [d[1] for d in desc], stream=st)
    finally:
        ctx.close()
