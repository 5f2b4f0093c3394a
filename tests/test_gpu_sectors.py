"""Sector tier on the GPU: dvda_pcm_hip_decode_sectors, dvda_mlp_hip_demux_sectors and
dvda_mlp_hip_pack_wav through the C ABI, exact, against the model of tests/sector_cases.py -- at every payload
alignment, packet count, chunk count and sector-count edge the kernels of csrc/pcm_unswizzle.h and csrc/wav_pack.h
branch on (tests/test_sector_model.py asserts that the table reaches them).

Every output buffer is larger than needed and pre-filled with a sentinel; every test asserts that nothing outside the
expected region changed: in front of an offset pointer, between the channel planes behind `frames`, behind the end.
The room behind the last plane holds whatever n sectors could decode to at most, so even a wrong count stays inside
the buffer the test owns."""
import ctypes

import numpy as np
import pytest

from tests import sector_cases as sc
from tests.test_pcm import _wide_samples

pytestmark = pytest.mark.gpu

GUARD = 64                       # words / bytes in front of every buffer; a multiple of 16 bytes either way
S32 = 0x5A5A5A5A
COUNTS = sc.COUNTS                # 1, 3, 4, 5, 4096, 4097, 5120, 5121


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    class G:
        pass
    g = G()
    g.torch, g.lib, g.dev = torch, pkg.hipdec.lib(), torch.device("cuda", 0)
    g.stream = torch.cuda.current_stream(g.dev).cuda_stream
    return g


def _dev(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a)).to(g.dev)


def _work(g, n):
    words = int(g.lib.dvda_pcm_hip_workspace_words(n))
    return g.torch.full((words + GUARD,), S32, dtype=g.torch.int32, device=g.dev), words


def _check_work(g, d_work, words, n, m):
    """d_work[s], d_work[n + s], d_work[2n] (include/dvda_mlp_hip.h), the bad count, the words behind the workspace"""
    w = d_work.cpu().numpy().view(np.uint32)
    assert np.array_equal(w[:n], m.counts.astype(np.uint32)), np.flatnonzero(w[:n] != m.counts)[:8]
    assert np.array_equal(w[n:2 * n + 1], m.base.astype(np.uint32)), np.flatnonzero(w[n:2 * n + 1] != m.base)[:8]
    assert (w[words:] == S32).all()
    total, bad = ctypes.c_uint64(), ctypes.c_uint32()
    assert g.lib.dvda_pcm_hip_result(d_work.data_ptr(), n, ctypes.byref(total), ctypes.byref(bad), g.stream) == 0
    assert total.value == m.base[-1] and bad.value == m.bad


def run_pcm(g, data, bps, ch, m, stride_extra=2, lead=0):
    """one dvda_pcm_hip_decode_sectors call checked against model m; stride = total + stride_extra, d_pcm `lead`
    words behind a 16-byte boundary"""
    n = len(data) // sc.SECTOR
    total = int(m.base[-1])
    stride = total + stride_extra
    room = n * 2 * (sc.SECTOR // (2 * ch * (bps // 8))) + GUARD          # the most n sectors can hold
    buf = g.torch.full((GUARD + lead + ch * stride + room,), S32, dtype=g.torch.int32, device=g.dev)
    d_sec = _dev(g, data)
    d_work, words = _work(g, n)
    assert buf.data_ptr() % 16 == 0 and d_sec.data_ptr() % 16 == 0
    rc = g.lib.dvda_pcm_hip_decode_sectors(d_sec.data_ptr(), n, bps, ch, buf.data_ptr() + 4 * (GUARD + lead), stride,
                                           d_work.data_ptr(), g.stream)
    assert rc == 0
    _check_work(g, d_work, words, n, m)
    out = buf.cpu().numpy()
    assert (out[:GUARD + lead] == S32).all(), "written in front of d_pcm"
    planes = out[GUARD + lead:GUARD + lead + ch * stride].reshape(ch, stride)
    assert np.array_equal(planes[:, :total], m.pcm), np.argwhere(planes[:, :total] != m.pcm)[:8]
    assert (planes[:, total:] == S32).all(), "written between the planes"
    assert (out[GUARD + lead + ch * stride:] == S32).all(), "written behind the last plane"
    return planes[:, :total].copy()


def run_mlp(g, data, m, cap=None):
    """one dvda_mlp_hip_demux_sectors call; returns the bytes below min(cap, total) and checks the rest untouched"""
    n = len(data) // sc.SECTOR
    total = int(m.base[-1])
    cap = total if cap is None else cap
    buf = g.torch.full((GUARD + len(data) + GUARD,), 0xA5, dtype=g.torch.uint8, device=g.dev)
    d_sec = _dev(g, data)
    d_work, words = _work(g, n)
    rc = g.lib.dvda_mlp_hip_demux_sectors(d_sec.data_ptr(), n, buf.data_ptr() + GUARD, cap, d_work.data_ptr(), g.stream)
    assert rc == 0
    _check_work(g, d_work, words, n, m)                 # the reported total is the full one whatever the cap
    out = buf.cpu().numpy()
    assert (out[:GUARD] == 0xA5).all(), "written in front of d_mlp"
    assert (out[GUARD + min(cap, total):] == 0xA5).all(), "written at or behind mlp_cap / the total"
    return out[GUARD:GUARD + min(cap, total)].copy()


def pcm_table(bps, ch, asg):
    """every shape of the table and every malformed sector (two of them side by side) in one run; the first and the
    last sector are malformed too, by a rule that moves with the layout"""
    secs = []
    rules = sc.RULES
    k = sc.LAYOUTS.index((bps, ch, asg))
    for i, (name, sh) in enumerate(sc.SECTOR_SHAPES.items()):
        secs.append(sc.pcm_sector(sh, bps, ch, asg, i)[0])
        if i < len(rules):
            secs.append(sc.malformed(rules[i], bps, asg))
    secs.insert(5, sc.malformed("codec", bps, asg))
    secs.insert(5, sc.malformed("ninth", bps, asg))
    secs.insert(0, sc.malformed(rules[(9 + k) % len(rules)], bps, asg))          # plen_lt_7 ... for layout 0 ...
    secs.append(sc.malformed(rules[(14 + k) % len(rules)], bps, asg))            # ninth ...
    return np.frombuffer(b"".join(secs), np.uint8).copy()


def mlp_table():
    data = ((np.arange(60000) * 73 + 5) >> 2).astype(np.uint8)
    good = sc.mlp_sectors(list(sc.MLP_SHAPES), data)
    rules = sc.rules_for(True)
    secs = []
    for i, s in enumerate(good):
        secs.append(s)
        if i < len(rules):
            secs.append(sc.malformed(rules[i], mlp=True))
    secs.insert(7, sc.malformed("overrun", mlp=True))
    secs.insert(7, sc.malformed("ninth", mlp=True))
    secs.insert(0, sc.malformed("ninth", mlp=True))
    secs.append(sc.malformed("hdr_gt_plen", mlp=True))
    return np.frombuffer(b"".join(secs), np.uint8).copy()


# ------------------------------------------------------------------------------------------------ PCM tier
@pytest.mark.parametrize("bps,ch,asg", sc.LAYOUTS)
def test_pcm_every_shape_and_rejection_rule(gpu, bps, ch, asg):
    """k_pcm_scan + k_pcm_unswizzle_t<CH, NB>: funnel shifts 0-3, 1/2/3/8 packets (frame0 carried from packet to
    packet), 0/1/63/64/65/most chunks, a payload up to byte 2047, every `return false` of walk_sector.  Then three
    more ways -- an odd stride, d_pcm 4 bytes off an 8-byte boundary, both: the scalar store path (vec_ok false)
    must give the planes of the vector path."""
    data = pcm_table(bps, ch, asg)
    m = sc.model_pcm(data, bps, ch)
    assert m.bad == len(sc.RULES) + 4 and m.base[-1] % 2 == 0
    vec = run_pcm(gpu, data, bps, ch, m, stride_extra=2, lead=0)
    for extra, lead in ((3, 0), (2, 1), (3, 1)):
        assert np.array_equal(run_pcm(gpu, data, bps, ch, m, stride_extra=extra, lead=lead), vec)


def _pcm_run(bps, ch, asg):
    period = [sc.pcm_sector(sh, bps, ch, asg, i)[0] for i, sh in enumerate(sc.SECTOR_SHAPES.values())]
    masks = [sc.payload_mask(s, 0xA0) for s in period]
    bad = {r: sc.malformed(r, bps, asg) for r in sc.RULES}
    return period, masks, bad


@pytest.mark.parametrize("bps,ch,asg", sc.LAYOUTS)
def test_pcm_sector_counts(gpu, bps, ch, asg):
    """1, 3, 4, 5 sectors (four per workgroup) and both sides of enqueue_exscan's change of form at 4096, with bad
    sectors first, in the middle, last, around sectors 256, 1024 and 4096 and every 317 sectors; the rules rotate with
    the layout and the count, so that over the layouts each rule lies at each of those places; every sector's payload
    differs, so one written at a wrong base is seen"""
    period, masks, bad = _pcm_run(bps, ch, asg)
    for n in COUNTS:
        plan = sc.bad_plan(n, sc.run_shift(sc.LAYOUTS.index((bps, ch, asg)), n), sc.RULES)
        data = sc.salted_run(period, masks, n, plan, bad).reshape(-1)
        m = sc.model_pcm(data, bps, ch)
        assert m.reasons == dict(plan)
        run_pcm(gpu, data, bps, ch, m, stride_extra=2 + (n & 1), lead=0)


def test_pcm_known_divergences_from_the_reference_reader(gpu):
    """Pinned, not fixed (tests/test_sector_model.py shows what the reference does with each): stray bytes behind the
    last packet, a parameter block that differs from the track's, a packet without a whole chunk -- the device call
    takes every sector for what its packets hold."""
    bps, ch, asg = 16, 2, 1
    plain = sc.pcm_sector(sc.SECTOR_SHAPES["off1"], bps, ch, asg, 9)[0]
    other = plain.replace(sc.params_block(bps, asg), sc.params_block(24, 12, 1))
    hole = sc.shape([sc.A(("c", 3, 0)), sc.A(("c", 0, 1)), sc.A(("c", 5, 0))])
    secs = [sc.pcm_sector(sc.SECTOR_SHAPES["stray1"], bps, ch, asg, 1)[0], plain, other,
            sc.pcm_sector(hole, bps, ch, asg, 2)[0], sc.pcm_sector(sc.SECTOR_SHAPES["stray5"], bps, ch, asg, 3)[0], plain]
    data = np.frombuffer(b"".join(secs), np.uint8).copy()
    m = sc.model_pcm(data, bps, ch)
    assert m.bad == 0 and (m.counts > 0).all()
    run_pcm(gpu, data, bps, ch, m)


# ------------------------------------------------------------------------------------------------ MLP demux
def test_mlp_every_shape_and_rejection_rule(gpu):
    """k_mlp_sector_scan + k_mlp_gather: packets of 0-3 bytes (shorter than the head run), 4-7, every (source & 3,
    dst & 3), several packets per sector, every rejection rule"""
    data = mlp_table()
    m = sc.model_mlp(data)
    assert m.bad == len(sc.rules_for(True)) + 4
    assert np.array_equal(run_mlp(gpu, data, m), m.mlp)


@pytest.fixture(scope="module")
def mlp_period():
    good = mlp_table().reshape(-1, sc.SECTOR)
    period = [bytes(s) for s in good if sc.walk(s, 0xA1)[0] is None][:40]
    return period, [sc.payload_mask(s, 0xA1) for s in period], {r: sc.malformed(r, mlp=True) for r in sc.rules_for(True)}


@pytest.mark.parametrize("shift", range(14))
def test_mlp_sector_counts(gpu, mlp_period, shift):
    """the sector counts and bad-sector places of test_pcm_sector_counts; over the 14 shifts each of the 14 rules
    lies at each named place"""
    period, masks, bad = mlp_period
    for n in COUNTS:
        plan = sc.bad_plan(n, sc.run_shift(shift, n), sc.rules_for(True))
        data = sc.salted_run(period, masks, n, plan, bad).reshape(-1)
        m = sc.model_mlp(data)
        assert m.reasons == dict(plan)
        assert np.array_equal(run_mlp(gpu, data, m), m.mlp)


def _byte_runs(m, x):
    """whether output byte x is stored by a head or tail byte run of its packet (k_mlp_gather: the bytes up to the
    first 4-byte aligned destination and those behind the packet's last whole dword) rather than as part of a dword"""
    for d, ln, off in m.packets:
        if d <= x < d + ln:
            head = min((4 - (d & 3)) & 3, ln)
            return x < d + head or x >= d + head + 4 * ((ln - head) >> 2)
    raise AssertionError(x)


def test_mlp_cap_smaller_than_the_payload(gpu):
    """mlp_cap (include/dvda_mlp_hip.h): no byte at or behind it is written; every byte below the last whole dword
    under it is right; the total reported stays the full one.  The 1-3 bytes between: the header promises no more
    than "right or untouched"; what the kernel does today is pinned exactly -- a byte of a packet's head or tail run
    is written, a byte of a dword that straddles the cap is not (the dword is dropped whole)."""
    data = mlp_table()
    m = sc.model_mlp(data)
    total = int(m.base[-1])
    in_packet = next(d + ln // 2 + 1 for d, ln, off in m.packets if ln >= 200 and d > 1000)
    in_head = next(d + 2 for d, ln, off in m.packets if d & 3 == 1 and ln >= 8 and d > 1000)
    in_tail = next(d + ln - 1 for d, ln, off in m.packets if (d + ln) & 3 == 3 and ln >= 12 and d > 1000)
    assert in_head & 3 == 3 and in_tail & 3 == 2             # two bytes of a three-byte head / tail run under the cap
    written = dropped = 0
    for cap in (total, total - 1, total - 2, total - 3, total - 4, total - 5, in_packet, in_packet + 1, in_head,
                in_tail):
        got = run_mlp(gpu, data, m, cap)
        whole = cap & ~3
        assert len(got) == cap and np.array_equal(got[:whole], m.mlp[:whole]), cap
        for x in range(whole, cap):
            if _byte_runs(m, x):
                assert got[x] == m.mlp[x], (cap, x)
                written += 1
            else:
                assert got[x] == 0xA5, (cap, x)
                dropped += m.mlp[x] != 0xA5                  # a dropped byte that the sentinel tells from a written one
    assert written >= 4 and dropped >= 4


def test_mlp_demux_then_decode_two_substreams(gpu, pkg, oracle):
    """a two-substream stream carried in multi-packet, odd-offset sectors: demux, then the decode, against the oracle"""
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=40)
    stream, frames = syn.stream(cfg, 31)
    names = ["mlp_big3", "eight", "mlp_dst_walk", "three_others", "mlp_big2", "most_off1", "two"]
    data = np.frombuffer(b"".join(sc.mlp_sectors(names, stream)), np.uint8).copy()
    m = sc.model_mlp(data)
    got = run_mlp(gpu, data, m)
    assert np.array_equal(got[:len(stream)], stream) and not got[len(stream):].any()
    pcm, infos = pkg.hipdec.decode_streams([got[:len(stream)]], lanes_per_segment=2)
    want, r, st = oracle.decode(stream, 6, frames)
    assert st == 0 and infos[0].status & ~pkg.hipdec.ST_BENIGN == 0
    assert np.array_equal(pcm[0], want)


# ------------------------------------------------------------------------------------------------ WAV payload
def run_wav(g, s, bits, stride, lead=0, out_lead=0, channels=None, frames=None, src=None, src_off=0):
    """one dvda_mlp_hip_pack_wav call.  s [ch, frames] lies in planes `stride` apart, d_pcm `lead` words behind a
    16-byte boundary, d_out `out_lead` bytes behind one; the words between the planes are noise the call must not
    read into the payload."""
    if src is None:
        ch, frames = s.shape
        rng = np.random.RandomState(stride + lead)
        src = rng.randint(-(1 << 31), 1 << 31, size=GUARD + lead + ch * stride + GUARD, dtype=np.int64).astype(np.int32)
        planes = src[GUARD + lead:GUARD + lead + ch * stride].reshape(ch, stride)
        planes[:, :frames] = s
        src_off = GUARD + lead
    else:
        ch = channels
    nbytes = frames * ch * (bits // 8)
    d_src = _dev(g, src)
    buf = g.torch.full((GUARD + out_lead + nbytes + GUARD,), 0xA5, dtype=g.torch.uint8, device=g.dev)
    assert d_src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    rc = g.lib.dvda_mlp_hip_pack_wav(d_src.data_ptr() + 4 * src_off, stride, ch, frames, bits,
                                     buf.data_ptr() + GUARD + out_lead, g.stream)
    assert rc == 0
    out = buf.cpu().numpy()
    assert (out[:GUARD + out_lead] == 0xA5).all(), "written in front of d_out"
    assert (out[GUARD + out_lead + nbytes:] == 0xA5).all(), "written behind the payload"
    assert np.array_equal(d_src.cpu().numpy(), src)
    return out[GUARD + out_lead:GUARD + out_lead + nbytes].copy()


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("ch", [1, 2, 3, 4, 5, 6])
def test_wav_pack_fast_generic_and_byte_paths(gpu, bits, ch):
    """k_pack_wav_fast<ch, bits> alone (1024, 2048 frames) and followed by a generic tail (1028, 2052, 1024 + 255,
    1024 + 257), with stride > frames; the same planes at stride & 3 != 0 and at d_pcm + 4, 8, 12 bytes (generic kernel
    only) and into d_out + 1, 2, 3 bytes (its byte path): one payload, the oracle's"""
    for frames in (1024, 2048, 1028, 2052, 1024 + 255, 1024 + 257):
        s = _wide_samples(ch, frames, frames + ch)
        want = sc.wav_payload(s, bits)
        stride = (frames + 40) & ~3
        assert stride % 4 == 0 and stride > frames
        fast = run_wav(gpu, s, bits, stride)
        assert np.array_equal(fast, want), (frames, np.flatnonzero(fast != want)[:8])
        for k in (1, 2, 3):
            assert np.array_equal(run_wav(gpu, s, bits, stride + k), want), (frames, "stride", k)
            assert np.array_equal(run_wav(gpu, s, bits, stride, lead=k), want), (frames, "d_pcm + %d" % (4 * k))
            assert np.array_equal(run_wav(gpu, s, bits, stride, out_lead=k), want), (frames, "d_out + %d" % k)
    for frames in (1, 255, 256, 257):                        # the generic kernel's 256-frame block edge
        s = _wide_samples(ch, max(frames, 4), frames + ch)[:, :frames].copy()
        want = sc.wav_payload(s, bits)
        for stride in (frames, frames + 3, frames + 8):
            assert np.array_equal(run_wav(gpu, s, bits, stride), want), (frames, stride)
        assert np.array_equal(run_wav(gpu, s, bits, frames + 1, lead=1, out_lead=3), want), frames


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("channels,served", [(2, 1), (3, 5), (5, 3), (6, 3), (6, 1023), (2, 2)])
def test_wav_pack_of_a_frame_major_source(gpu, bits, channels, served):
    """the disc tier's call for a frame-major buffer: one "channel" of left * channels values, stride 4, starting
    served * channels values into the buffer -- an element offset that is no multiple of 4 for all but the last case"""
    left = 1500
    inter = np.ascontiguousarray(_wide_samples(channels, served + left, served + bits).T.reshape(-1))
    src = np.concatenate([np.full(GUARD, S32, np.int64).astype(np.int32), inter, np.zeros(GUARD, np.int32)])
    got = run_wav(gpu, None, bits, 4, channels=1, frames=left * channels, src=src, src_off=GUARD + served * channels)
    want = sc.wav_payload(inter[served * channels:].reshape(1, -1), bits)
    assert ((served * channels) & 3 != 0) or (channels, served) == (2, 2)
    assert np.array_equal(got, want)
