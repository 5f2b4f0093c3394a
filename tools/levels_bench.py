"""The level report on the bench's headline titles (synthetic, 6 ch 96 kHz, 512 access units each, interleaved int32
output, one job), in alternating rounds:

    a  index + blocking decode per step, as tools/digest_bench.py times it
    b  the same plus dvda_pcm_hip_levels of every stream, enqueued behind the decode
    c  the same plus dvda_pcm_hip_crc32 (the digest) instead
    d  the device-to-host copy of the int32 PCM into pinned memory: what a host-side scan would need first

and, between two device events each: the report's kernels alone, and dvda_mlp_hip_pack_wav over the same PCM -- the
yardstick for a kernel that only streams these bytes -- with the int32 bytes per second both read.
The planar layout's kernels are timed once more behind a planar decode of the same titles.

Prints one JSON line; some reports are checked against tests/levels_model.py over the PCM copied back once, outside the
timed rounds.

    python tools/levels_bench.py [--streams 1024] [--aus 512] [--steps 20] [--bits 24]
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
from tests import levels_model as lm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bits", type=int, default=24)
    ap.add_argument("--check", type=int, default=8, help="streams whose report is compared with the model")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    L = hd.lib()
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=args.aus)
    flat, offs, sizes, frames = syn.batch(cfg, 1, args.streams)
    n, nb = args.streams, args.bits // 8
    batch = hd.Batch(packed=(flat, offs, sizes))
    dev, st = batch.dev, batch.current_stream
    rows = frames.astype(np.int64)
    total_frames = int(rows.sum())
    pcm_bytes = total_frames * 6 * 4
    payload = total_frames * 6 * nb
    sz = ctypes.sizeof(hd.Levels)

    def setup(layout):
        out = hd.PcmRegions(rows, [6] * n, layout)
        ctx = hd.Context(0, n, n * ((args.aus + 7) // 8) + 64, 0, layout)
        rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
        rec["off"], rec["stride"], rec["frames"], rec["channels"] = out.out_off, rows, rows, 6
        d_desc = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)
        d_lvl = torch.zeros((n, sz), dtype=torch.uint8, device=dev)
        d_work = torch.empty(hd.pcm_levels_workspace_words(n, total_frames), dtype=torch.int32, device=dev)

        def levels():
            hd._check(L.dvda_pcm_hip_levels(out.d_pcm.data_ptr(), layout, args.bits, d_desc.data_ptr(), n, total_frames,
                                            d_lvl.data_ptr(), d_work.data_ptr(), d_work.numel(), st), "dvda_pcm_hip_levels")

        def decode():
            ctx.index_batch(batch, st)
            ctx.decode(*out.ptrs, st)

        return out, ctx, d_desc, d_lvl, decode, levels

    out, ctx, d_desc, d_lvl, decode, levels = setup(hd.PCM_INTERLEAVED)
    d_pcm, out_off = out.d_pcm, out.out_off
    d_cwork = torch.empty(hd.pcm_crc32_workspace_words(n, payload), dtype=torch.int32, device=dev)
    d_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    d_nbytes = torch.zeros(n, dtype=torch.int64, device=dev)
    d_wav = torch.zeros(payload + 64, dtype=torch.uint8, device=dev)
    h_copy = torch.empty(pcm_bytes // 4, dtype=torch.int32).pin_memory()
    assert out_off[0] == 0 and d_pcm.numel() >= total_frames * 6

    def digest():
        hd._check(L.dvda_pcm_hip_crc32(d_pcm.data_ptr(), hd.PCM_INTERLEAVED, args.bits, d_desc.data_ptr(), n, payload,
                                       d_crc.data_ptr(), d_nbytes.data_ptr(), d_cwork.data_ptr(), d_cwork.numel(), st),
                  "dvda_pcm_hip_crc32")

    def pack():
        # frame-major values already are in payload order: one "channel" of all of them (as the disc tier packs them)
        hd._check(L.dvda_mlp_hip_pack_wav(d_pcm.data_ptr(), 4, 1, total_frames * 6, args.bits, d_wav.data_ptr(), st),
                  "dvda_mlp_hip_pack_wav")

    def decode_levels():
        decode()
        levels()

    def decode_digest():
        decode()
        digest()

    def copy():
        h_copy.copy_(d_pcm[:pcm_bytes // 4], non_blocking=True)

    def between_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"a_decode": decode, "b_decode_levels": decode_levels, "c_decode_digest": decode_digest, "d_copy_int32": copy}
    kernels = {"levels_kernels": levels, "pack_wav_yardstick": pack, "digest_kernels": digest}
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

    infos = ctx.stream_info(stream=st)
    bad = sum(1 for inf in infos if inf.status & ~hd.ST_BENIGN)
    got = hd.levels_list(d_lvl)
    checked = 0
    for i in np.linspace(0, n - 1, min(n, args.check)).astype(int):
        p = d_pcm[int(out_off[i]):int(out_off[i]) + int(rows[i]) * 6].cpu().numpy().reshape(-1, 6).T
        assert got[i] == lm.levels(p, args.bits), "stream %d: the device's report is not the model's" % i
        checked += 1

    # the planar layout, once: the same titles decoded into planes, the report's kernels alone
    ctx.close()
    p_out, p_ctx, _, p_lvl, p_decode, p_levels = setup(hd.PCM_PLANAR)
    p_decode()
    planar_ms = [between_events(p_levels) for _ in range(args.warmup + args.steps)][args.warmup:]
    assert hd.levels_list(p_lvl) == got, "the planar layout's reports differ from the interleaved one's"
    p_ctx.close()

    res = {"streams": n, "aus": args.aus, "bits": args.bits, "int32_bytes": pcm_bytes, "non_benign": bad,
           "reports_checked_against_model": checked, "planar_equals_interleaved": True, "unit": "ms per step"}
    for name, v in times.items():
        res[name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3),
                     "max_ms": round(float(np.max(v)), 3)}
    kernel_ms["levels_kernels_planar"] = planar_ms
    for name, v in kernel_ms.items():
        km = float(np.median(v))
        res[name] = {"median_ms": round(km, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                     "int32_read_GB_per_s": round(pcm_bytes / km / 1e6, 1)}
    res["copy_GB_per_s"] = round(pcm_bytes / float(np.median(times["d_copy_int32"])) / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
