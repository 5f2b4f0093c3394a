"""The compare of two PCM buffers on the bench's headline titles (synthetic, 6 ch 96 kHz, 512 access units each, int32
output, one job): two rips of the same titles, each decoded on a context of its own into a buffer of its own.  In
alternating rounds:

    a  index + blocking decode of both batches
    b  the same plus dvda_pcm_hip_compare of every stream pair, enqueued behind the decodes
    c  the device-to-host copies of both int32 PCM buffers into pinned memory: what a host-side compare would need first

and, between two device events each: the compare's kernels alone, frame-major against frame-major, planar against
frame-major and planar against planar (two more, planar decodes of the same titles), and dvda_pcm_hip_levels over the
bytes of the two frame-major buffers, one call each -- the yardstick for a report that only streams them (DESIGN.md
section 13), with the int32 bytes per second each reads, both sides counted.

The decodes write the same PCM, so the timed compares find no difference; some values of side B are then changed on the
device, outside the timed rounds, and some diffs are checked against tests/compare_model.py over the PCM copied back.

Prints one JSON line.

    python tools/compare_bench.py [--streams 1024] [--aus 512] [--steps 20] [--bits 0]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libdvd_audio_amd as pkg  # noqa: E402
from tests import compare_model as cm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bits", type=int, default=0)
    ap.add_argument("--check", type=int, default=8, help="stream pairs whose diff is compared with the model")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    L = hd.lib()
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=args.aus)
    flat, offs, sizes, frames = syn.batch(cfg, 1, args.streams)
    n = args.streams
    batch = hd.Batch(packed=(flat, offs, sizes))
    dev, st = batch.dev, batch.current_stream
    rows = frames.astype(np.int64)
    total_frames = int(rows.sum())
    pcm_bytes = total_frames * 6 * 4
    sz = ctypes.sizeof(hd.Diff)

    def side(layout):
        """a context, its regions and their descriptors on the device"""
        out = hd.PcmRegions(rows, [6] * n, layout)
        ctx = hd.Context(0, n, n * ((args.aus + 7) // 8) + 64, 0, layout)
        rec = hd._desc_records([(o, r, r, 6) for o, r in zip(out.out_off, rows)])
        d_desc = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)

        def decode():
            ctx.index_batch(batch, st)
            ctx.decode(*out.ptrs, st)

        return ctx, out, d_desc, decode

    ctx_a, out_a, desc_a, decode_a = side(hd.PCM_INTERLEAVED)
    ctx_b, out_b, desc_b, decode_b = side(hd.PCM_INTERLEAVED)
    ctx_p, out_p, desc_p, decode_p = side(hd.PCM_PLANAR)
    ctx_q, out_q, desc_q, decode_q = side(hd.PCM_PLANAR)
    d_diff = torch.zeros((n, sz), dtype=torch.uint8, device=dev)
    d_work = torch.empty(hd.pcm_compare_workspace_words(n, total_frames), dtype=torch.int32, device=dev)
    d_lvl = torch.zeros((n, ctypes.sizeof(hd.Levels)), dtype=torch.uint8, device=dev)
    d_lwork = torch.empty(hd.pcm_levels_workspace_words(n, total_frames), dtype=torch.int32, device=dev)
    h_copy = [torch.empty(pcm_bytes // 4, dtype=torch.int32).pin_memory() for _ in range(2)]
    assert out_a.out_off[0] == 0 and out_a.d_pcm.numel() >= total_frames * 6

    def compare(a=out_a, la=hd.PCM_INTERLEAVED, da=desc_a, b=out_b, lb=hd.PCM_INTERLEAVED, db=desc_b):
        hd._check(L.dvda_pcm_hip_compare(a.d_pcm.data_ptr(), la, da.data_ptr(), b.d_pcm.data_ptr(), lb, db.data_ptr(), n,
                                         args.bits, total_frames, d_diff.data_ptr(), d_work.data_ptr(), d_work.numel(), st),
                  "dvda_pcm_hip_compare")

    def compare_planar():
        compare(out_p, hd.PCM_PLANAR, desc_p)

    def compare_planar_planar():
        compare(out_p, hd.PCM_PLANAR, desc_p, out_q, hd.PCM_PLANAR, desc_q)

    def levels_both():
        for out, desc in ((out_a, desc_a), (out_b, desc_b)):
            hd._check(L.dvda_pcm_hip_levels(out.d_pcm.data_ptr(), hd.PCM_INTERLEAVED, 24, desc.data_ptr(), n, total_frames,
                                            d_lvl.data_ptr(), d_lwork.data_ptr(), d_lwork.numel(), st),
                      "dvda_pcm_hip_levels")

    def decode_two():
        decode_a()
        decode_b()

    def decode_two_compare():
        decode_two()
        compare()

    def copies():
        for h, out in zip(h_copy, (out_a, out_b)):
            h.copy_(out.d_pcm[:pcm_bytes // 4], non_blocking=True)

    def between_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    decode_p()
    decode_q()
    legs = {"a_decode_two": decode_two, "b_decode_two_compare": decode_two_compare, "c_copy_two_int32": copies}
    kernels = {"compare_kernels_frame_major": compare, "compare_kernels_planar_vs_frame_major": compare_planar,
               "compare_kernels_planar_vs_planar": compare_planar_planar,
               "levels_kernels_both_buffers": levels_both}
    times = {k: [] for k in legs}
    kernel_ms = {k: [] for k in kernels}
    for k in range(args.warmup + args.steps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append((time.perf_counter() - t) * 1e3)
        for name, fn in kernels.items():
            ms = between_events(fn)
            if k >= args.warmup:
                kernel_ms[name].append(ms)

    bad = sum(1 for c in (ctx_a, ctx_b, ctx_p, ctx_q) for inf in c.stream_info(stream=st) if inf.status & ~hd.ST_BENIGN)
    compare()
    clean = hd.diff_list(d_diff)
    assert all(d["diff_frames"] == 0 and d["compared"] == int(r) for d, r in zip(clean, rows)), "two decodes of one batch differ"
    for fn in (compare_planar, compare_planar_planar):
        fn()
        assert hd.diff_list(d_diff) == clean, "a planar decode differs from the frame-major one"

    # side B changed in places: a value in every 4099th, a stretch of whole frames in the checked streams
    picks = [int(i) for i in np.linspace(0, n - 1, min(n, args.check)).astype(int)]
    out_b.d_pcm[::4099] ^= 0x40
    for i in picks:
        o, r = int(out_b.out_off[i]), int(rows[i])
        out_b.d_pcm[o + 6 * (r // 3):o + 6 * (r // 3 + 5000)] += 3
    checked = 0
    results = []
    for fn, out_x, planar in ((compare, out_a, False), (compare_planar, out_p, True)):
        fn()
        got = hd.diff_list(d_diff)
        results.append(got)
        for i in picks:
            r = int(rows[i])
            x = out_x.d_pcm[int(out_x.out_off[i]):int(out_x.out_off[i]) + r * 6].cpu().numpy()
            x = x.reshape(6, r) if planar else x.reshape(r, 6).T
            y = out_b.d_pcm[int(out_b.out_off[i]):int(out_b.out_off[i]) + r * 6].cpu().numpy().reshape(r, 6).T
            want = cm.diff(x, y, args.bits)
            assert got[i] == want, "pair %d: the device's diff is not the model's" % i
            assert want["diff_frames"] >= 5000 and want["runs"] > 1
            checked += 1
    assert results[0] == results[1]
    for c in (ctx_a, ctx_b, ctx_p, ctx_q):
        c.close()

    res = {"streams": n, "aus": args.aus, "bits": args.bits, "int32_bytes_per_side": pcm_bytes, "non_benign": bad,
           "diffs_checked_against_model": checked, "planar_equals_frame_major": True, "unit": "ms per step"}
    for name, v in times.items():
        res[name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3),
                     "max_ms": round(float(np.max(v)), 3)}
    for name, v in kernel_ms.items():
        km = float(np.median(v))
        res[name] = {"median_ms": round(km, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                     "int32_read_GB_per_s": round(2 * pcm_bytes / km / 1e6, 1)}
    res["b_minus_a_ms"] = round(res["b_decode_two_compare"]["median_ms"] - res["a_decode_two"]["median_ms"], 3)
    res["copy_GB_per_s"] = round(2 * pcm_bytes / float(np.median(times["c_copy_two_int32"])) / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
