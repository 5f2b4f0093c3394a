"""The energy report on the GPU (dvda_pcm_hip_energy, dvda_mlp_hip_pcm_energy; csrc/pcm_energy.h): what the device
reports of int32 PCM in either layout is tests/energy_model of the same values.  Every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from tests import energy_model as em
from tests import presentation_model as pm
from tests.stream_tools import frame_offsets, is_major_sync
from tests.test_conceal_model import make_stream as conceal_stream
from tests.test_gpu_levels import FILL, LAYOUTS, _layout, place
from tests.test_presentation_model import make_stream

pytestmark = pytest.mark.gpu

P = em.PIECE
CHANNELS = [1, 2, 3, 6, 8]
FRAMES = [1, 63, 64, 65, P - 1, P, P + 1, 3 * P + 5]
_PCM, _WANT = {}, {}


def rail_pcm(rng, ch, frames):
    """full-range int32 with runs of -2^31 and of 2^31 - 1"""
    pcm = rng.integers(-2 ** 31, 2 ** 31, (ch, frames), dtype=np.int64)
    for c in range(ch):
        a = int(rng.integers(0, frames))
        pcm[c, a:a + 70] = -2 ** 31
        b = int(rng.integers(0, frames))
        pcm[c, b:b + 9] = 2 ** 31 - 1
    return pcm.astype(np.int32)


def sweep_pcm(ch, frames):
    """computed once, shared, never written to"""
    if (ch, frames) not in _PCM:
        _PCM[(ch, frames)] = rail_pcm(np.random.default_rng(100 * ch + frames), ch, frames)
        _PCM[(ch, frames)].setflags(write=False)
    return _PCM[(ch, frames)]


def want_of(ch, frames, B, lead):
    key = (ch, frames, B, lead)
    if key not in _WANT:
        _WANT[key] = em.energy_fast(sweep_pcm(ch, frames), B, lead)
    return _WANT[key]


def run(hd, flat, layout, desc, B, lead=None, **kw):
    import torch
    d_pcm = torch.from_numpy(flat).to(torch.device("cuda", 0))
    return hd.energy_lists(*hd.pcm_energy(d_pcm, _layout(hd, layout), desc, B, lead=lead, **kw))


def test_fast_model_is_the_model():
    """(the sweep's reference is the numpy form of the model: here against the one written with Python integers)"""
    pcm = sweep_pcm(3, P + 1)
    for B, lead in ((64, None), (100, 1), (4410, 4409)):
        assert em.energy_fast(pcm, B, lead) == em.energy(pcm, B, lead)
    assert em.energy(pcm, 5000)[0]["sq_hi"][0] > 0


@pytest.mark.parametrize("B", [64, 100, 4096, 4410, 5000])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sweep(pkg, layout, B):
    """every channel count and length, off at each of the four dword alignments, planar strides odd; the leads NULL, then
    1 and B - 1 side by side in one call"""
    hd = pkg.hipdec
    shapes = [(ch, f) for ch in CHANNELS for f in FRAMES]
    pcms = [sweep_pcm(ch, f) for ch, f in shapes]
    slack = [37 + (f & 1) for _, f in shapes] if layout == "planar" else [37]
    flat, desc = place(pcms, layout, slack, off_mod=[0, 1, 2, 3, 3, 2, 1])
    assert {d[0] % 4 for d in desc} == {0, 1, 2, 3}
    if layout == "planar":
        assert all(d[1] & 1 for d in desc)
    got, counts = run(hd, flat, layout, desc, B)
    for i, (ch, f) in enumerate(shapes):
        assert counts[i] == em.nblocks(f, B) and got[i] == want_of(ch, f, B, None), (i, ch, f)
    leads = [(1, B - 1)[i % 2] for i in range(len(shapes))] + [(B - 1, 1)[i % 2] for i in range(len(shapes))]
    got, counts = run(hd, flat, layout, desc + desc, B, lead=leads)
    for i, (ch, f) in enumerate(shapes + shapes):
        assert counts[i] == em.nblocks(f, B, leads[i]) and got[i] == want_of(ch, f, B, leads[i]), (i, ch, f, leads[i])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_long_blocks_and_a_lead_out_of_range(pkg, layout):
    """a block of several pieces whose sums carry far into sq_hi; a lead of 0 and one above B: no blocks"""
    hd = pkg.hipdec
    B = 3 * P + 100
    p = np.full((2, 2 * B + 7), -2 ** 31, np.int32)
    p[1, ::3] = 2 ** 31 - 1
    flat, desc = place([p, p, p, p], layout, [1])
    got, counts = run(hd, flat, layout, desc, B, lead=[B, P + 1, 0, B + 1])
    assert counts == [3, 3, 0, 0] and got[2] == got[3] == []
    assert got[0] == em.energy_fast(p, B) and got[1] == em.energy_fast(p, B, P + 1)
    assert got[0][0]["sq_hi"][0] == B // 4 and got[0][0]["peak"][:2] == [2 ** 31, 2 ** 31]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_33_streams_caps_bound_and_canaries(pkg, layout):
    """33 streams in one call, some empty or not taken; one with a cap below its block count; a max_total_frames too small
    for the last streams; canaries around d_blocks and the workspace; a workspace of 0xFF bytes, then a second run"""
    import torch
    hd = pkg.hipdec
    L = hd.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(33)
    B, n = 100, 33
    pcms, chans = [], []
    for i in range(n):
        ch = int(rng.integers(1, 9))
        frames = 0 if i in (4, 17) else int(rng.integers(1, 3000))
        pcms.append(rail_pcm(rng, ch, frames) if frames else np.zeros((ch, 0), np.int32))
        chans.append(0 if i == 9 else 9 if i == 21 else ch)
    flat, desc = place(pcms, layout, [3], off_mod=[1, 0, 3, 2])
    desc = [(d[0], d[1], d[2], chans[i]) for i, d in enumerate(desc)]
    leads = [int(rng.integers(1, B + 1)) for _ in range(n)]
    taken = [1 <= chans[i] <= 8 and desc[i][2] > 0 for i in range(n)]
    full = [em.energy_fast(pcms[i], B, leads[i]) if taken[i] else [] for i in range(n)]
    pieces = [em.pieces_of_stream(desc[i][2], B, leads[i]) if taken[i] else 0 for i in range(n)]
    base = np.concatenate([[0], np.cumsum(pieces)])
    # the bound: the list ends inside stream 27
    bound = next(b for b in range(0, 100000, 50) if base[27] <= b // P + b // B + 2 * n < base[28])
    max_tiles = bound // P + bound // B + 2 * n
    inside = [int(base[i + 1]) <= max_tiles for i in range(n)]
    assert all(inside[:27]) and not any(inside[i] for i in range(27, n) if taken[i]) and sum(taken[27:]) >= 4
    short = 12
    assert taken[short] and len(full[short]) >= 4
    room = [len(b) for b in full]
    caps = list(room)
    caps[short] = 2
    first = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    want_counts = [len(full[i]) if inside[i] else 0 for i in range(n)]

    size, guard = ctypes.sizeof(hd.EnergyBlock), 2
    words = hd.pcm_energy_workspace_words(n, bound, B)
    d_pcm = torch.from_numpy(flat).to(dev)
    d_desc = torch.from_numpy(hd._desc_records(desc).view(np.uint8).reshape(-1)).to(dev)
    d_lead = torch.tensor(leads, dtype=torch.int32).to(dev)
    d_off = torch.from_numpy(first[:n] + guard).to(dev)
    d_cap = torch.tensor(caps, dtype=torch.int64).to(dev)
    results = []
    for fill in (-1, 0):
        d_blocks = torch.full(((int(first[n]) + 2 * guard) * size,), 0xEE, dtype=torch.uint8, device=dev)
        d_nb = torch.full((n,), -7, dtype=torch.int64, device=dev)
        d_work = torch.full((words + 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_work[16:16 + words] = fill
        rc = L.dvda_pcm_hip_energy(d_pcm.data_ptr(), _layout(hd, layout), d_desc.data_ptr(), n, B, d_lead.data_ptr(), bound,
                                   d_blocks.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_nb.data_ptr(),
                                   d_work.data_ptr() + 64, words, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        work = d_work.cpu().numpy()
        assert (work[:16] == 0x5A5A5A5A).all() and (work[16 + words:] == 0x5A5A5A5A).all()
        results.append((d_blocks.cpu().numpy().reshape(-1, size), d_nb.cpu().numpy().tolist()))
    (raw, counts), (raw2, counts2) = results
    assert counts == counts2 == want_counts and np.array_equal(raw, raw2)
    assert counts[short] == len(full[short]) > caps[short]
    assert (raw[:guard] == 0xEE).all() and (raw[guard + int(first[n]):] == 0xEE).all()
    for i in range(n):
        rows = raw[guard + int(first[i]):guard + int(first[i + 1])]
        written = min(counts[i], caps[i])
        got = [hd.EnergyBlock.from_buffer_copy(rows[j].tobytes()).as_dict() for j in range(written)]
        assert got == full[i][:written], i
        assert (rows[written:] == 0xEE).all(), i            # behind a cap, and a stream outside the bound: untouched


_ORACLE = {}


def golden(pkg, oracle, name):
    """the two small recipes of tests/golden: (stream bytes, the oracle's PCM)"""
    if name not in _ORACLE:
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
        b = np.ascontiguousarray(z["mlp"])
        ch, f = z["pcm"].shape
        want, r, st = oracle.decode(b, ch, f)
        assert st == 0 and r == f and np.array_equal(want, z["pcm"])
        _ORACLE[name] = (b, want)
    return _ORACLE[name]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_after_a_decode(pkg, oracle, layout):
    hd = pkg.hipdec
    cases = [golden(pkg, oracle, "recipe_6ch_96k"), golden(pkg, oracle, "recipe_2ch_96k")]
    for B in (64, 9600):
        pcm, infos, blocks = hd.decode_streams([b for b, _ in cases], layout=_layout(hd, layout), energy=B)
        for (b, want), got, inf, blk in zip(cases, pcm, infos, blocks):
            assert inf.status & ~hd.ST_BENIGN == 0 and np.array_equal(got, want)
            assert blk == em.energy_fast(want, B) and len(blk) == em.nblocks(want.shape[1], B) > 0
    # beside the digest and the level report: appended last
    res = hd.decode_streams([cases[1][0]], layout=_layout(hd, layout), crc32=True, levels=24, energy=4800)
    assert len(res) == 5 and res[4] == [em.energy_fast(cases[1][1], 4800)] and res[3][0]["frames"] == cases[1][1].shape[1]


def test_default_return_shape_is_unchanged(pkg, oracle):
    hd = pkg.hipdec
    b, _ = golden(pkg, oracle, "recipe_2ch_96k")
    assert len(hd.decode_streams([b])) == 2 and len(hd.decode_streams([b], energy=None)) == 2
    assert len(hd.decode_streams([b], levels=24)) == 3 and len(hd.decode_streams_concealed([b])) == 3
    assert len(hd.decode_streams([b], energy=64)) == 3 and len(hd.decode_streams_concealed([b], energy=64)) == 4


def test_presentation_and_conceal_mode(pkg, oracle):
    """frames and channels as stream_info reports them: the presentation's k channels, conceal mode's composed stream"""
    hd = pkg.hipdec
    B = 480
    b, _ = make_stream(pkg, "CHAINED", 0)
    pcm, infos, blocks = hd.decode_streams([b], presentation=hd.PRESENT_SUBSTREAM0, energy=B)
    want, frames, ost, k = pm.expect(b, oracle)
    assert ost == 0 and int(infos[0].channels) == k == 2 and int(infos[0].pcm_frames) == frames
    assert blocks[0] == em.energy_fast(want, B) and blocks[0][0]["sq_lo"][2:] == [0] * 6

    c, _, _ = conceal_stream(pkg, 2, "CHAINED")
    offs = frame_offsets(c)
    assert any(is_major_sync(c, o) for o in offs)
    mid = c.copy()
    mid[offs[19] + (offs[20] - offs[19]) // 2] ^= 0x10
    pcm, infos, spans, blocks = hd.decode_streams_concealed([mid], layout=hd.PCM_INTERLEAVED, energy=B)
    assert infos[0].status & hd.ST_CONCEALED and spans[0] and spans[0][0][1] > 0
    assert pcm[0].shape == (int(infos[0].channels), int(infos[0].pcm_frames))
    assert blocks[0] == em.energy_fast(pcm[0], B)


def test_wav_context_and_capacity(pkg, oracle):
    hd = pkg.hipdec
    cases = [golden(pkg, oracle, "recipe_2ch_96k"), golden(pkg, oracle, "recipe_6ch_96k")]
    B = 1000
    batch = hd.Batch([b for b, _ in cases])
    st = batch.current_stream
    ctx = hd.Context(0, batch.n, max(64, batch.total // 64))
    try:
        ctx.index_batch(batch, st)
        infos = ctx.stream_info(stream=st)
        out = hd.PcmRegions.for_infos(infos, hd.PCM_PLANAR, 0)
        ctx.decode(*out.ptrs, st)
        want = [em.energy_fast(w, B) for _, w in cases]
        need = sum(len(w) for w in want)
        assert ctx.pcm_energy(*out.ptrs, B, stream=st) == want
        assert ctx.pcm_energy(*out.ptrs, B, stream=st, cap_blocks=need) == want
        # one block short: ECAPACITY, the count needed in host_first[n], nothing else written
        first = (ctypes.c_uint64 * 3)(7, 7, 7)
        arr = (hd.EnergyBlock * need)()
        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
        rc = hd.lib().dvda_mlp_hip_pcm_energy(ctx._h, *out.ptrs, B, arr, need - 1, first, batch.n, st)
        assert rc == -4 and list(first) == [7, 7, need] and bytes(arr) == b"\xee" * ctypes.sizeof(arr)
        with pytest.raises(hd.HipError, match="ECAPACITY"):
            ctx.pcm_energy(*out.ptrs, B, stream=st, cap_blocks=need - 1)
        for bad in (63, (1 << 24) + 1):
            with pytest.raises(hd.HipError, match="EINVAL"):
                ctx.pcm_energy(*out.ptrs, bad, stream=st)
        ctx.set_pcm_layout(hd.PCM_WAV24)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_energy(*out.ptrs, B, stream=st)
    finally:
        ctx.close()
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.decode_streams([cases[0][0]], layout=hd.PCM_WAV16, energy=B)
    import torch
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.pcm_energy(torch.zeros(64, dtype=torch.int32, device="cuda:0"), hd.PCM_WAV24, [(0, 8, 8, 1)], 64)
