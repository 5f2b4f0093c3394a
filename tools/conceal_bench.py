"""Conceal mode on the bench's headline titles (synthetic, 6 ch 96 kHz, 512 access units each, interleaved output):
step time (index + blocking decode) with conceal mode off, on for the clean batch, and on with 1 % of the titles damaged
(one payload bit flipped in one access unit each).  Prints one JSON line.

    python tools/conceal_bench.py [--streams 1024] [--aus 512] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libdvd_audio_amd as pkg  # noqa: E402
from tests.stream_tools import frame_offsets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--damaged", type=float, default=0.01, help="fraction of titles damaged once each")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=args.aus)
    flat, offs, sizes, frames = syn.batch(cfg, 1, args.streams)
    n = args.streams
    dmg = flat.copy()
    hit = np.linspace(0, n - 1, max(1, int(round(n * args.damaged)))).astype(int)
    for i in hit:
        o = int(offs[i])
        fo = frame_offsets(flat[o:o + int(sizes[i])])
        j = len(fo) // 2 + 3
        dmg[o + fo[j] + (fo[j + 1] - fo[j]) // 2] ^= 0x10
    # (room for silence longer than what the bytes say)
    out = hd.PcmRegions([int(f) + 65536 for f in frames], [6] * n, hd.PCM_INTERLEAVED)
    segs = n * ((args.aus + 7) // 8) + 64
    res = {"streams": n, "aus": args.aus, "damaged_titles": len(hit), "unit": "ms per step (index + decode)"}
    for name, buf, conceal in (("off_clean", flat, 0), ("on_clean", flat, 1), ("on_damaged", dmg, 1), ("off_clean_2", flat, 0)):
        ctx = hd.Context(0, n, segs, 0, hd.PCM_INTERLEAVED)
        ctx.set_conceal(conceal)
        batch = hd.Batch(packed=(buf, offs, sizes))
        st = batch.current_stream
        times = []
        for k in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ctx.index_batch(batch, st)
            ctx.decode(*out.ptrs, st)
            torch.cuda.synchronize()
            if k >= args.warmup:
                times.append((time.perf_counter() - t) * 1e3)
        infos = ctx.stream_info(stream=st)
        conc = sum(1 for inf in infos if inf.status & hd.ST_CONCEALED)
        bad = sum(1 for inf in infos if inf.status & ~(hd.ST_BENIGN | hd.ST_CONCEALED))
        res[name] = {"median_ms": round(float(np.median(times)), 3), "min_ms": round(float(np.min(times)), 3),
                     "max_ms": round(float(np.max(times)), 3), "concealed": conc, "non_benign": bad}
        ctx.close()
        del batch
    print(json.dumps(res))


if __name__ == "__main__":
    main()
