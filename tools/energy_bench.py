"""The energy report on the bench's headline titles (synthetic, 6 ch 96 kHz, 512 access units each, interleaved int32
output, one job), in alternating rounds:

    a  index + blocking decode per step, as tools/levels_bench.py times it
    b  the same plus dvda_pcm_hip_energy of every stream (blocks of --block frames), enqueued behind the decode
    c  the same plus dvda_pcm_hip_levels instead: the yardstick, a report that reads the same PCM once
    d  the device-to-host copy of the int32 PCM into pinned memory: what a host-side meter would need first

and, between two device events each: the energy report's kernels alone and the level report's kernels alone, with the
int32 bytes per second both read.  The planar layout's kernels are timed once more behind a planar decode of the same
titles.

Prints one JSON line; some streams' blocks are checked against tests/energy_model.py over the PCM copied back once,
outside the timed rounds.

    python tools/energy_bench.py [--streams 1024] [--aus 512] [--steps 20] [--block 9600]
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
from tests import energy_model as em  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block", type=int, default=9600)
    ap.add_argument("--check", type=int, default=8, help="streams whose blocks are compared with the model")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    L = hd.lib()
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=args.aus)
    flat, offs, sizes, frames = syn.batch(cfg, 1, args.streams)
    n, B = args.streams, args.block
    batch = hd.Batch(packed=(flat, offs, sizes))
    dev, st = batch.dev, batch.current_stream
    rows = frames.astype(np.int64)
    total_frames = int(rows.sum())
    pcm_bytes = total_frames * 6 * 4
    counts = [hd.energy_nblocks(int(f), B) for f in rows]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    size = ctypes.sizeof(hd.EnergyBlock)

    def setup(layout):
        out = hd.PcmRegions(rows, [6] * n, layout)
        ctx = hd.Context(0, n, n * ((args.aus + 7) // 8) + 64, 0, layout)
        rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
        rec["off"], rec["stride"], rec["frames"], rec["channels"] = out.out_off, rows, rows, 6
        d_desc = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)
        d_blocks = torch.zeros((int(first[n]), size), dtype=torch.uint8, device=dev)
        d_off = torch.from_numpy(first[:n].copy()).to(dev)
        d_cap = torch.tensor(counts, dtype=torch.int64).to(dev)
        d_nb = torch.zeros(n, dtype=torch.int64, device=dev)
        d_work = torch.empty(hd.pcm_energy_workspace_words(n, total_frames, B), dtype=torch.int32, device=dev)
        d_lvl = torch.zeros((n, ctypes.sizeof(hd.Levels)), dtype=torch.uint8, device=dev)
        d_lwork = torch.empty(hd.pcm_levels_workspace_words(n, total_frames), dtype=torch.int32, device=dev)

        def energy():
            hd._check(L.dvda_pcm_hip_energy(out.d_pcm.data_ptr(), layout, d_desc.data_ptr(), n, B, None, total_frames,
                                            d_blocks.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_nb.data_ptr(),
                                            d_work.data_ptr(), d_work.numel(), st), "dvda_pcm_hip_energy")

        def levels():
            hd._check(L.dvda_pcm_hip_levels(out.d_pcm.data_ptr(), layout, 24, d_desc.data_ptr(), n, total_frames,
                                            d_lvl.data_ptr(), d_lwork.data_ptr(), d_lwork.numel(), st), "dvda_pcm_hip_levels")

        def decode():
            ctx.index_batch(batch, st)
            ctx.decode(*out.ptrs, st)

        return out, ctx, (d_blocks, d_nb), decode, energy, levels

    out, ctx, res_i, decode, energy, levels = setup(hd.PCM_INTERLEAVED)
    d_pcm, out_off = out.d_pcm, out.out_off
    h_copy = torch.empty(pcm_bytes // 4, dtype=torch.int32).pin_memory()
    assert out_off[0] == 0 and d_pcm.numel() >= total_frames * 6

    def decode_energy():
        decode()
        energy()

    def decode_levels():
        decode()
        levels()

    def copy():
        h_copy.copy_(d_pcm[:pcm_bytes // 4], non_blocking=True)

    def between_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"a_decode": decode, "b_decode_energy": decode_energy, "c_decode_levels": decode_levels, "d_copy_int32": copy}
    kernels = {"energy_kernels": energy, "levels_kernels": levels}
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
    got, got_counts = hd.energy_lists(res_i[0], [int(v) for v in first], res_i[1])
    assert got_counts == counts
    checked = 0
    for i in np.linspace(0, n - 1, min(n, args.check)).astype(int):
        p = d_pcm[int(out_off[i]):int(out_off[i]) + int(rows[i]) * 6].cpu().numpy().reshape(-1, 6).T
        assert got[i] == em.energy_fast(p, B), "stream %d: the device's blocks are not the model's" % i
        checked += 1

    # the planar layout, once: the same titles decoded into planes, the report's kernels alone
    ctx.close()
    p_out, p_ctx, res_p, p_decode, p_energy, _ = setup(hd.PCM_PLANAR)
    p_decode()
    planar_ms = [between_events(p_energy) for _ in range(args.warmup + args.steps)][args.warmup:]
    assert torch.equal(res_p[0], res_i[0]), "the planar layout's blocks differ from the interleaved one's"
    p_ctx.close()

    res = {"streams": n, "aus": args.aus, "block_frames": B, "blocks": int(first[n]), "int32_bytes": pcm_bytes,
           "non_benign": bad, "streams_checked_against_model": checked, "planar_equals_interleaved": True,
           "unit": "ms per step"}
    for name, v in times.items():
        res[name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3),
                     "max_ms": round(float(np.max(v)), 3)}
    kernel_ms["energy_kernels_planar"] = planar_ms
    for name, v in kernel_ms.items():
        km = float(np.median(v))
        res[name] = {"median_ms": round(km, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                     "int32_read_GB_per_s": round(pcm_bytes / km / 1e6, 1)}
    res["copy_GB_per_s"] = round(pcm_bytes / float(np.median(times["d_copy_int32"])) / 1e6, 1)
    res["energy_over_levels_kernels"] = round(res["energy_kernels"]["median_ms"] / res["levels_kernels"]["median_ms"], 2)
    res["energy_kernels_over_copy"] = round(res["energy_kernels"]["median_ms"] / res["d_copy_int32"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
