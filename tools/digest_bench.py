"""The PCM digest on the bench's headline titles (synthetic, 6 ch 96 kHz, 512 access units each, interleaved int32
output, one job), in alternating rounds:

    a  index + blocking decode per step, as tools/conceal_bench.py times it
    b  the same plus dvda_pcm_hip_crc32 of every stream's 24-bit WAV payload, enqueued behind the decode
    c  the device-to-host copy of as many bytes as that payload has, into pinned memory: what the digest replaces
    d  the digest's kernels alone, between two device events, and the payload bytes per second that makes

Prints one JSON line; every CRC is checked against zlib over the PCM copied back once, outside the timed rounds.

    python tools/digest_bench.py [--streams 1024] [--aus 512] [--steps 20] [--bits 24]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libdvd_audio_amd as pkg  # noqa: E402
from tests import digest_model as dm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bits", type=int, default=24)
    ap.add_argument("--check", type=int, default=8, help="streams whose CRC is compared with zlib")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=args.aus)
    flat, offs, sizes, frames = syn.batch(cfg, 1, args.streams)
    n, nb = args.streams, args.bits // 8
    batch = hd.Batch(packed=(flat, offs, sizes))
    dev, st = batch.dev, batch.current_stream
    rows = frames.astype(np.int64)
    out = hd.PcmRegions(rows, [6] * n, hd.PCM_INTERLEAVED)
    d_pcm, out_off = out.d_pcm, out.out_off
    ctx = hd.Context(0, n, n * ((args.aus + 7) // 8) + 64, 0, hd.PCM_INTERLEAVED)

    rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
    rec["off"], rec["stride"], rec["frames"], rec["channels"] = out_off, rows, rows, 6
    payload = int((rows * 6 * nb).sum())
    d_desc = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)
    d_work = torch.empty(hd.pcm_crc32_workspace_words(n, payload), dtype=torch.int32, device=dev)
    d_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    d_nbytes = torch.zeros(n, dtype=torch.int64, device=dev)
    d_copy = torch.zeros(payload, dtype=torch.uint8, device=dev)
    h_copy = torch.empty(payload, dtype=torch.uint8).pin_memory()

    def decode():
        ctx.index_batch(batch, st)
        ctx.decode(*out.ptrs, st)

    def digest():
        hd._check(hd.lib().dvda_pcm_hip_crc32(d_pcm.data_ptr(), hd.PCM_INTERLEAVED, args.bits, d_desc.data_ptr(), n, payload,
                                              d_crc.data_ptr(), d_nbytes.data_ptr(), d_work.data_ptr(), d_work.numel(), st),
                  "dvda_pcm_hip_crc32")

    def decode_digest():
        decode()
        digest()

    def copy():
        h_copy.copy_(d_copy, non_blocking=True)

    legs = {"a_decode": decode, "b_decode_digest": decode_digest, "c_copy_payload": copy}
    times = {k: [] for k in legs}
    kernel_ms = []
    for k in range(args.warmup + args.steps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append((time.perf_counter() - t) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        digest()
        e1.record()
        torch.cuda.synchronize()
        if k >= args.warmup:
            kernel_ms.append(e0.elapsed_time(e1))

    infos = ctx.stream_info(stream=st)
    bad = sum(1 for inf in infos if inf.status & ~hd.ST_BENIGN)
    got = hd.crc_list(d_crc, d_nbytes)
    checked = 0
    for i in np.linspace(0, n - 1, min(n, args.check)).astype(int):
        p = d_pcm[int(out_off[i]):int(out_off[i]) + int(rows[i]) * 6].cpu().numpy().reshape(-1, 6).T
        pay = dm.wav_payload(p, args.bits)
        assert got[i] == (zlib.crc32(pay), len(pay)), "stream %d: the device's CRC is not zlib's" % i
        checked += 1
    res = {"streams": n, "aus": args.aus, "bits": args.bits, "payload_bytes": payload, "non_benign": bad,
           "crc_checked_against_zlib": checked, "unit": "ms per step"}
    for name, v in times.items():
        res[name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3),
                     "max_ms": round(float(np.max(v)), 3)}
    km = float(np.median(kernel_ms))
    res["d_digest_kernels"] = {"median_ms": round(km, 3), "min_ms": round(float(np.min(kernel_ms)), 3),
                               "payload_GB_per_s": round(payload / km / 1e6, 1),
                               "int32_read_GB_per_s": round(int((rows * 6 * 4).sum()) / km / 1e6, 1)}
    res["copy_GB_per_s"] = round(payload / float(np.median(times["c_copy_payload"])) / 1e6, 1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
