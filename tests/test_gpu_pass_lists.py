"""The seven PCM passes on the GPU at the places of the shared tile list their own files do not reach
(csrc/pcm_tiles.h, csrc/pcm_report_run.h; the cases and the pass adapters: tests/pass_list_cases.py; the premises of every
case: tests/test_pass_lists_model.py).  What the device writes and reports is the model's of the same values; nothing
else in an output buffer changes.  Every comparison is exact."""
import numpy as np
import pytest

from tests import pass_list_cases as plc

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
THREADS = plc.kernel_constants()["THREADS"]
CROSSED = [("planar", "interleaved"), ("interleaved", "planar")]


def same(st, got, reports, want_reports=None, want_out=None, mask=None):
    """the reports, then the whole output buffer (where `mask` says so)"""
    want_reports = st.reports if want_reports is None else want_reports
    assert len(reports) == len(want_reports)
    if reports != want_reports:
        i = next(i for i, (g, w) in enumerate(zip(reports, want_reports)) if g != w)
        assert reports[i] == want_reports[i], (i, st.streams[i].pcm.shape, st.streams[i].kind, int(st.base[i]))
    if got is not None:
        want_out = st.expect if want_out is None else want_out
        differs = got != want_out
        if mask is not None:
            differs &= mask
        bad = np.flatnonzero(differs)
        assert bad.size == 0, (bad[:8], [d for d in st.true_out if d[0] <= bad[0]][-1:])


# ---- A: every channel count
@pytest.mark.parametrize("case", plc.channel_passes(), ids=lambda c: c[0])
def test_every_channel_count(pkg, case):
    """ch = 1 .. 8 in one call, each stream one full tile and a ragged second tile that is no multiple of the kernel's
    work item: every chunk size and partial chunk of the resampler and the decimator, every lane mapping"""
    hd = pkg.hipdec
    _, p, (lay_in, lay_out) = case
    st = p.stage(hd, plc.channel_cases(p), lay_in, lay_out)
    got, reports = p.call(hd, st)
    same(st, got, reports)


# ---- B: a long list
def canaried(p, hd, st, fill):
    """a run on a workspace of exactly the words the pass asks for, filled with `fill`, between canaries"""
    import torch
    words = p.workspace_words(hd, st.n, st.total)
    d_work = torch.full((words + 32,), CANARY, dtype=torch.int32, device="cuda:0")
    d_work[16:16 + words] = fill
    got, reports = p.call(hd, st, max_total=st.total, work=d_work[16:16 + words])
    work = d_work.cpu().numpy()
    assert (work[:16] == CANARY).all() and (work[16 + words:] == CANARY).all()
    return got, reports


@pytest.mark.parametrize("lay_in,lay_out", CROSSED)
@pytest.mark.parametrize("name", plc.ALL)
def test_long_list(pkg, name, lay_in, lay_out):
    """4200 streams in one call: the scan in its three-launch form, every workgroup's second turn (a third, where the
    kernel has 2048 workgroups) with another channel count than its first, find_stream over 4200 bases; then twice more
    on a dirtied workspace of exactly the words asked for; then with a bound that cuts a stream behind the first turn"""
    hd = pkg.hipdec
    p = plc.list_pass(name)
    streams, info = plc.long_list(p)
    st = p.stage(hd, streams, lay_in, lay_out if p.writes else None)
    assert list(st.base) == list(info.base)
    got, reports = p.call(hd, st)
    same(st, got, reports)
    for fill in (-1, 0):
        got, reports = canaried(p, hd, st, fill)
        same(st, got, reports)
    cut, want_reports, out = p.cut(st, info.max_total)
    assert cut == info.cut
    got, reports = p.call(hd, st, max_total=info.max_total)
    same(st, got, reports, want_reports, *(out or ()))
    assert want_reports[cut] == p.behind() != st.reports[cut]


# ---- C: a long stream
@pytest.mark.parametrize("lay_in,lay_out", CROSSED)
@pytest.mark.parametrize("content", ["mixed", "tail"])
@pytest.mark.parametrize("name", plc.WRITERS)
def test_long_stream(pkg, name, content, lay_in, lay_out):
    """one stream of THREADS + 1 tiles: the join's second turn.  "tail": the only values that clip lie in the last
    tile, so a join that stopped at THREADS records would report none"""
    hd = pkg.hipdec
    p = plc.list_pass(name)
    streams = plc.long_stream(p, content)
    st = p.stage(hd, streams, lay_in, lay_out, off_in=(1, 2), off_out=(3, 1), slack_in=(5,), slack_out=(3,))
    clipped = st.reports[0]["clipped"]
    if content == "tail":
        if name == "resample":          # (the CPU file has it from a bound; here the whole model is at hand)
            assert clipped == p.slice_model(hd, streams[0].pcm, THREADS)[1]
        assert clipped[0] > 0
    else:
        assert clipped[0] > THREADS
    got, reports = p.call(hd, st)
    same(st, got, reports)


# ---- D: the count fields at their maximum
@pytest.mark.parametrize("lay_out", plc.LAYOUTS)
@pytest.mark.parametrize("name", plc.WRITERS)
def test_count_fields_at_their_maximum(pkg, name, lay_out):
    """every value of all eight channels of a full tile clips: each 16-bit field of the two count words holds the
    tile's frame count, and no field carries into its neighbour"""
    hd = pkg.hipdec
    p = plc.clip_pass(name)
    streams = plc.all_clip(p)
    st = p.stage(hd, streams, plc.OTHER[lay_out], lay_out, off_in=(1,), off_out=(2,))
    assert st.reports[0]["clipped"] == [p.out_tile + 1] * 8           # the model says so first
    got, reports = p.call(hd, st)
    assert reports[0]["clipped"] == [p.out_tile + 1] * 8
    same(st, got, reports)
