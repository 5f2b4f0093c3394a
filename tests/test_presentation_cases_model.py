"""The premises of tests/presentation_cases.py, on the CPU: the copy sweep reaches every (dst phase, src - dst phase) pair
and every body class it claims -- asserted from the model's own walk of the built streams, so the GPU sweep
(tests/test_gpu_presentation_edges.py) cannot pass by missing one --, the clamp cases take every clamp of pp_unit, the
decodable cases decode in the model with the status the table names, and the stripped streams agree with the compiled
reference (live where it is built, else by the digests of tests/golden/presentation_digests.json)."""
import collections

import numpy as np
import pytest

from tests import index_model as im
from tests import oracle_lib
from tests import presentation_cases as pc
from tests import presentation_model as pm
from tests import stream_tools
from tests.test_presentation_model import PRES_DIGESTS


def _source_is_resolvable(b):
    flat, offs, lens, total = pc.source(b)
    ix = im.expect(flat, total, offs, lens)
    return all(x.resolvable for x, s in zip(ix.streams, b.streams) if pm.substreams_of(s))


# ------------------------------------------------------------------------------------------------ (a) the sweep

@pytest.fixture(scope="module")
def sweep(pkg):
    b = pc.batch(pkg.synth, "sweep")
    return b, pc.walk(b)


def test_sweep_reaches_every_pair_in_every_class(sweep):
    b, recs = sweep
    hit = collections.defaultdict(set)
    for r in recs:
        hit[pc.body_class(r.n, r.dst)].add(pc.pair(r))
        if r.n == pc.MAX_BODY:
            hit["9"].add(pc.pair(r))
    for cls in ("2", "4", "5", "7"):
        want = {(d, e) for d, e in pc.ALL_PAIRS if pc.exists(cls, d)}
        assert len(want) == (48 if cls == "2" else 64)
        assert want <= hit[cls], "class %s misses the pairs %r" % (cls, sorted(want - hit[cls]))
    for cls in ("1", "3", "6a", "6b", "8", "9"):
        assert {e for _, e in hit[cls]} == set(range(0, 16, 2)), "class %s: src - dst phases %r" % (cls, sorted(hit[cls]))
    # class 2 is left out only where no such body exists: an even n with 0 < n < h needs h >= 4
    assert [d for d in range(0, 16, 2) if not pc.exists("2", d)] == [0, 14]
    # the lane loop's turns: 64 whole chunks end the first, 65 begin the second, 129 the third
    assert all(((r.n - ((16 - r.dst) & 15)) >> 4) >= 129 for r in recs if pc.body_class(r.n, r.dst) == "8")


def test_sweep_crosses_both_directory_sizes_on_sync_and_plain_units(sweep):
    b, recs = sweep
    shapes = {(r.dir0, r.dir1, r.sync) for r in recs[1:]}
    assert shapes >= {(a, c, s) for a in (2, 4) for c in (2, 4) for s in (0, 28)}
    for cls in ("2", "4", "5", "7"):
        mine = {(r.dir0, r.dir1, r.sync) for r in recs if pc.body_class(r.n, r.dst) == cls}
        assert len(mine) == 8, cls
    assert not any(r.clamped for r in recs), "the sweep's units are whole"
    assert max(im.unit_size(s, p) for s in b.streams for p in stream_tools.frame_offsets(s)) == pc.MAX_UNIT


def test_hand_made_streams_are_framed_as_built_and_only_indexed(pkg):
    syn = pkg.synth
    for group in pc.HAND_MADE:
        for b in pc.batches(syn, group).values():
            assert b.decode is None
            with pytest.raises(AssertionError):
                pc.expected_info(b, 0, None)
            assert _source_is_resolvable(b), b.name
            ix = pc.inner_index(b)
            assert all(x.resolvable for x in ix.streams), b.name
            _, _, lens, _ = pc.present_buffer(b)
            for s, x, n in zip(b.streams, ix.streams, lens):
                assert pm.strip(s)[1] == 2 and x.bytes_consumed == n == len(pm.strip(s)[0])
                assert x.mlp_frames == len(stream_tools.frame_offsets(s))


# ------------------------------------------------------------------------------------------------ (b) the clamps

def test_clamp_cases_take_every_clamp(pkg):
    b = pc.batch(pkg.synth, "clamps")
    recs = [r for r in pc.walk(b) if r.stream == 0]
    s = b.streams[0]
    size = {r.unit: im.unit_size(s, p) for r, p in zip(recs, stream_tools.frame_offsets(s))}
    by_size = collections.defaultdict(set)
    for r in recs:
        by_size[size[r.unit], r.sync].add(r.clamped)
    assert by_size[4, 0] == {frozenset(["no_dir"])} and by_size[32, 28] == {frozenset(["no_dir"])}
    for plain, sync in ((6, 34), (8, 36), (10, 38)):
        assert by_size[plain, 0] and by_size[sync, 28], (plain, sync)
    labels = collections.Counter(c for r in recs for c in r.clamped)
    assert set(labels) == {"no_dir", "dir0", "no_dir1", "dir1", "end0"}
    # an extra-word flag on a word that is the unit's last two bytes: substream 0's, and substream 1's
    assert frozenset(["dir0", "no_dir1", "end0"]) in by_size[6, 0] and frozenset(["dir0", "no_dir1", "end0"]) in by_size[34, 28]
    assert any("dir1" in c and "dir0" not in c for c in by_size[8, 0])
    # substream_end_0 beyond the unit with the directory whole, on a plain and on a sync unit
    whole = [r for r in recs if r.clamped == frozenset(["end0"]) and size[r.unit] > 40]
    assert {r.sync for r in whole} == {0, 28}
    # substream_end_1 < substream_end_0: no clamp of the strip's (it never reads substream 1's end), the body is whole
    offs = stream_tools.frame_offsets(s)
    low = []
    for r in recs:
        p = offs[r.unit]
        d = p + 4 + r.sync
        if not r.clamped and r.dir0 and r.dir1:
            w0 = ((int(s[d]) << 8) | int(s[d + 1])) & 0xFFF
            w1 = ((int(s[d + r.dir0]) << 8) | int(s[d + r.dir0 + 1])) & 0xFFF
            if w1 < w0:
                low.append(r)
    assert {r.sync for r in low} == {0, 28} and all(r.n == 40 for r in low)
    # good units between them, and the stream goes on to its end
    assert sum(1 for r in recs if not r.clamped) > 20 and pm.consumed(s) == len(s)


# ------------------------------------------------------------------------------------------------ (c) large bodies

def test_large_bodies_are_large_and_decode_clean(pkg, oracle):
    b = pc.batch(pkg.synth, "large")
    recs = pc.walk(b)
    assert len(b.streams) == 8
    for i in range(8):
        n = [r.n for r in recs if r.stream == i]
        assert len(n) == 12 and min(n) > 1040, (i, min(n))                  # every body: a second turn of the lane loop
        info, pcm = pc.expected_info(b, i, oracle)
        assert (info["channels"], info["pcm_frames"], info["mlp_frames"], info["status"]) == (5, 1920, 12, 0)
        assert pcm.shape == (5, 1920)
    assert sum(1 for r in recs if r.n > 2064) >= 8                          # several: a third turn
    assert {pc.body_class(r.n, r.dst) for r in recs} >= {"8"}
    assert {int(s[11]) & 0x1F for s in b.streams} == {12, 20}


# ------------------------------------------------------------------------------------------------ (d) one substream

def test_one_substream_segments_lie_at_every_phase(pkg, oracle):
    b = pc.batch(pkg.synth, "one_substream")
    flat, offs, lens, total = pc.source(b)
    buf, poffs, plens, _ = pc.present_buffer(b)
    assert plens == [len(s) for s in b.streams]
    for i, s in enumerate(b.streams):
        assert pm.substreams_of(s) == 1 and pm.consumed(s) == len(s)
        assert np.array_equal(pm.strip(s)[0], s) and np.array_equal(buf[poffs[i]:poffs[i] + plens[i]], s)
        info, pcm = pc.expected_info(b, i, oracle)
        nch = b.decode["nch"][i]
        want, frames, st = oracle.decode(s, nch, info["pcm_frames"])
        assert st == 0 and info["status"] == 0 and info["channels"] == nch and np.array_equal(pcm, want)
    six = b.streams[0]
    syncs = stream_tools.major_syncs(six)
    assert {p % 16 for p in syncs} == set(range(0, 16, 2))
    sizes = np.diff(syncs + [len(six)])
    assert len(sizes) == 9 and (sizes > 1024).sum() >= 8, sizes


# ------------------------------------------------------------------------------------------------ (e) mixed findings

def test_mixed_batch_is_what_it_says(pkg, oracle):
    b = pc.batch(pkg.synth, "mixed")
    kinds = b.decode["kinds"]
    _, _, plens, _ = pc.present_buffer(b)
    assert kinds.count("none") == 2 and kinds.count("envelope") == 2 and kinds.count("cut") == 4
    for i, (s, kind) in enumerate(zip(b.streams, kinds)):
        if kind != "good":
            assert kinds[i - 1] == "good" and kinds[i + 1] == "good"        # good streams on both sides
        if kind == "none":
            assert plens[i] == 0 and pm.substreams_of(s) == 0
        elif kind == "envelope":
            assert plens[i] == 0 and pm.strip(s) [2] == pm.ST_ENVELOPE and pm.substreams_of(s) == 2
            assert im.single(s).status == 0                                  # the full decode's index has nothing to say
        else:
            info, pcm = pc.expected_info(b, i, oracle)
            assert info["status"] == (im.TRUNCATED if kind == "cut" else 0) and pcm.shape[1] == info["pcm_frames"] > 0
            if kind == "cut":
                x = im.single(s)
                assert x.status == im.TRUNCATED and x.bytes_consumed == info["bytes_consumed"] < len(s)
    cuts = [b.streams[i] for i, k in enumerate(kinds) if k == "cut"]
    assert [len(c) - pm.consumed(c) for c in cuts[:3]] == [2, 20, 34]
    assert [len(im.single(c).live) for c in cuts] == [1, 1, 2, 2]          # 34 bytes and more: the last major sync stands whole


# ------------------------------------------------------------------------------------------------ (f) sync edges

def test_sync_edges_give_the_frame_counts_the_table_names(pkg, oracle):
    b = pc.batch(pkg.synth, "sync")
    ix = pc.inner_index(b)
    for i, (name, (pres, full)) in enumerate(pc.SYNC_CLAIMS.items()):
        s = b.streams[i]
        pcm, frames, ost, k = pm.expect(s, oracle)
        assert (frames, ost) == pres and k == 2, name
        if full is not None:
            assert oracle.decode(s, 6, 1920)[1:] == full, name
        assert im.single(s).resolvable and ix.streams[i].resolvable
    src = [im.single(s) for s in b.streams]
    # false syncs behind substream 0 vanish; those in substream 0's bytes are candidates of the inner index again, and
    # still say two substreams
    assert src[0].segments == 3 + 8 and ix.streams[0].segments == 3
    assert src[1].segments == 3 + 5 and ix.streams[1].segments == 3 + 5
    buf, poffs, plens, _ = pc.present_buffer(b)
    false = [int(c) for j, c in enumerate(ix.cands) if ix.seg[j] is None and poffs[1] <= c < poffs[1] + plens[1]]
    assert len(false) == 5 and all(int(buf[c + 20]) >> 4 == 2 for c in false)
    assert all(int(buf[g.off + 20]) >> 4 == 1 for g in ix.seg if g is not None)
    # the unit whose major sync differs in the assignment alone: dropped by the full decode's index, live in the inner one
    assert (src[2].status, src[2].mlp_frames) == (im.SYNC_CHANGE, 23) and (ix.streams[2].status, ix.streams[2].mlp_frames) == (0, 24)
    assert (src[3].status, src[3].mlp_frames) == (im.SYNC_CHANGE, 23) and (ix.streams[3].status, ix.streams[3].mlp_frames) == (im.SYNC_CHANGE, 23)


# ------------------------------------------------------------------------------------------------ (g) geometry

def test_geometry_streams_are_the_shortest_that_give_k(pkg):
    syn = pkg.synth
    for n in (255, 256, 257, 1025, 16385):
        b = pc.batch(syn, "geometry%d" % n)
        flat, offs, lens, total = pc.source(b)
        assert len(b.streams) == n and total < (1 << 20) and set(lens.tolist()) == {42}
    s = b.streams[-1]
    assert pm.strip(s)[1] == 2 and len(pm.strip(s)[0]) == 40
    for cut in (s[:40].copy(), ):
        cut[1] = 20                                     # five bytes of substream 0: bits 40-43 are not there
        cut[33] = 2
        assert pm.strip(cut)[2] == pm.ST_ENVELOPE
    assert len({x.tobytes() for x in b.streams}) == n


# ------------------------------------------------------------------------------------------------ (h) buffer reuse

def test_the_big_batch_leaves_a_major_sync_behind_the_small_one(pkg, oracle):
    syn = pkg.synth
    big, small = pc.batch(syn, "reuse_big"), pc.batch(syn, "reuse_small")
    bbuf, _, _, bbound = pc.present_buffer(big)
    sbuf, soffs, slens, sbound = pc.present_buffer(small)
    lo, hi = soffs[-1] + slens[-1], sbound + 64
    assert hi < bbound
    stale = [int(c) for c in im.candidates(bbuf, bbound) if lo <= c and c + 32 <= hi]
    assert stale, "no major sync of the big batch inside the small batch's zero range"
    assert not sbuf[lo:].any()
    for seq in pc.REUSE_SEQUENCES.values():
        assert seq[-1][1] == 1
    for b in (big, small):
        for i in range(len(b.streams)):
            info, pcm = pc.expected_info(b, i, oracle)
            assert info["status"] == 0 and info["channels"] == 2 and pcm.shape == (2, info["pcm_frames"])


# ------------------------------------------------------------------------------------------------ the getter's symbol

def test_present_read_is_declared_exported_and_bound(pkg):
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "dvda_mlp_hip.h")).read()
    assert re.search(r"int dvda_mlp_hip_present_read\(dvda_mlp_hip_ctx \*ctx,", h) and "Diagnostic" in h
    so = pkg._build.build_hip()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert "dvda_mlp_hip_present_read" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "dvda_mlp_hip_present_read" in pkg.hipdec.EXPORTS and hasattr(pkg.hipdec.Context, "present_read")
    assert len(pkg.hipdec.lib().dvda_mlp_hip_present_read.argtypes) == 9


# ------------------------------------------------------------------------------------------------ the reference

def _reference_cases(syn):
    out = []
    for group in ("large", "sync"):
        for b in pc.batches(syn, group).values():
            for i, name in enumerate(b.decode["names"]):
                out.append((b, i, "edges_%s_%s" % (group, name)))
    return out


def test_stripped_streams_agree_with_the_reference(pkg, oracle, monkeypatch):
    monkeypatch.setattr(oracle_lib, "REF_DIGESTS", PRES_DIGESTS)
    for b, i, key in _reference_cases(pkg.synth):
        s, k, st = pm.strip(b.streams[i])
        pcm, frames, ost, pk = pm.expect(b.streams[i], oracle)
        assert st == 0 and pk == k
        rate = b.decode["rate"]
        assert oracle_lib.same_as_reference(
            key, (pcm, frames), lambda: oracle_lib.Reference().decode(s, pm.IDENTITY_ASSIGNMENT[k], rate, 2, frames)), key
