#!/usr/bin/env python3
"""Full decode against the 2-channel presentation (dvda_mlp_hip_set_presentation) on two of bench.py's shapes:

    two_substreams   recipe titles, ch 0-1 | ch 2-5
    disc_profile     chained titles, two substreams, parameters on every block, mixed code books

One job, two contexts, the two settings in alternating rounds on the same device buffers: per setting the wall time of
a step (dvda_mlp_hip_index + dvda_mlp_hip_decode + stream synchronize), the device time of the decode call, and for the
presentation the strip kernels' own device time with the bytes they walked and wrote.

    python tools/presentation_bench.py [--streams 1024] [--aus 512] [--steps 20] [--rounds 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def shapes(syn, aus):
    SF = syn.SF
    return [("two_substreams", syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=aus)),
            ("disc_profile", syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=aus, profile=1,
                                          features=SF["DISC"] | SF["CHAINED"] | SF["FIRRAND"] | SF["MIXBOOKS"]))]


class Side:
    """one setting: its context, its PCM buffer"""

    def __init__(self, hd, torch, nseg, presentation, batch, st):
        self.hd, self.torch, self.st, self.batch = hd, torch, st, batch
        self.ctx = hd.Context(0, batch.n, nseg, 0, hd.PCM_INTERLEAVED)
        self.ctx.set_presentation(presentation)
        self.ctx.index_batch(batch, st)
        self.out = hd.PcmRegions.for_infos(self.ctx.stream_info(stream=st), hd.PCM_INTERLEAVED, slack=16)
        self.channels = self.out.channels[0]
        self.step()
        infos = self.ctx.stream_info(stream=st)
        bad = [i for i, inf in enumerate(infos) if inf.status & ~hd.ST_BENIGN]
        if bad:
            raise SystemExit("presentation_bench: stream %d status %#x" % (bad[0], infos[bad[0]].status))
        self.frames = int(sum(int(i.pcm_frames) for i in infos))
        self.wall, self.steps, self.rounds = 0.0, 0, []

    def step(self):
        self.ctx.index_batch(self.batch, self.st)
        self.ctx.decode(*self.out.ptrs, self.st)

    def run(self, steps):
        self.torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.torch.cuda.synchronize()
        dt = time.perf_counter() - t
        self.wall += dt
        self.steps += steps
        self.rounds.append(dt / steps * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import libdvd_audio_amd as pkg
    hd, syn = pkg.hipdec, pkg.synth
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    lines = ["presentation_bench: %d titles x %d access units, %d rounds x %d steps per setting, %s"
             % (a.streams, a.aus, a.rounds, a.steps, torch.cuda.get_device_name(0))]
    for name, cfg in shapes(syn, a.aus):
        flat, offs, sizes, frames = syn.batch(cfg, 1, a.streams)
        batch = hd.Batch(packed=(flat, offs, sizes))
        total = batch.total
        nseg = a.streams * ((a.aus + cfg.restart_interval - 1) // cfg.restart_interval + 2) + 1024
        sides = [("full", Side(hd, torch, nseg, hd.PRESENT_FULL, batch, st)),
                 ("presentation", Side(hd, torch, nseg, hd.PRESENT_SUBSTREAM0, batch, st))]
        for _, s in sides:
            s.run(3)                                # warm-up (the index's graph is captured on the third call)
            s.wall, s.steps, s.rounds = 0.0, 0, []
            s.ctx.kernel_time()
        strip = []
        for _ in range(a.rounds):
            for label, s in sides:
                s.run(a.steps)
                if label == "presentation":
                    strip.append(s.ctx.present_time())
        lines.append("%s: %.1f MB compressed, %d PCM frames per title set" % (name, total / 1e6, sides[0][1].frames))
        res = {}
        for label, s in sides:
            dec_ms, _ = s.ctx.decode_time()
            ms = s.wall / s.steps * 1e3
            res[label] = ms
            lines.append("  %-12s %d ch  %8.3f ms/step (index + decode, wall; rounds %s)  decode call %8.3f ms (device)  "
                         "%8.1f Mframes/s" % (label, s.channels, ms, " ".join("%.3f" % r for r in s.rounds), dec_ms,
                                              s.frames / ms / 1e3))
        ms_strip = float(np.median([t[0] for t in strip]))
        b_in, b_out = strip[-1][1], strip[-1][2]
        lines.append("  strip kernels %.3f ms (device, median of %d): source %.1f MB -> presentation %.1f MB (%.1f %%), "
                     "%.1f GB/s of presentation bytes read + written"
                     % (ms_strip, len(strip), b_in / 1e6, b_out / 1e6, 100.0 * b_out / b_in, 2.0 * b_out / ms_strip / 1e6))
        lines.append("  presentation / full = %.3f" % (res["presentation"] / res["full"]))
        for _, s in sides:
            s.ctx.close()
        del sides, batch
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
