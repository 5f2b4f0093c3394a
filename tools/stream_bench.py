#!/usr/bin/env python3
"""tools/stream_bench.py [chained] [--group N [--group-only]] [--reps R] -- speed of tier B (the mlp.h mirror) fed
one 6-ch / 96 kHz title in PES-payload sized packets (2 011 bytes), calling the C entry points directly (no Python list
building): Msamples/s and ms per call.  Diagnostic.

Without --group: one lone decoder (dvda_hip_mlpdecoder_decode_packet).  With --group N: N copies of the title, each
member's from its own seed, through ONE group (dvda_hip_mlpdecoder_group_decode_packets: a call feeds every member its
next packet), and beside it, in the same process and in turn, the same packets through N lone decoders fed one after
the other (--group-only: without them, for a profiler run whose kernel statistics are the group's alone).  The first of
the R repetitions (default 2) warms up; every later one prints a line."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdvd_audio_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("chained", nargs="?", choices=["chained"])
ap.add_argument("--group", type=int, default=0, metavar="N")
ap.add_argument("--group-only", action="store_true")
ap.add_argument("--reps", type=int, default=2, metavar="R")
args = ap.parse_args()

syn, hip = pkg.synth, pkg.hipdec
chained = args.chained is not None
cfg = syn.make_cfg(assignment=12, rate_code=1, n_aus=1024, **(dict(profile=1, features=syn.SF["CHAINED"]) if chained else {}))
L = hip.lib()
PACKET = 2011
what = " (chained title)" if chained else ""


def pieces_of(seed):
    b, frames = syn.stream(cfg, seed)
    return [np.ascontiguousarray(b[o:o + PACKET]) for o in range(0, len(b), PACKET)], frames


def lone_in_turn(titles):
    """every title through its own lone decoder, call k of all of them before call k + 1 -> (PCM frames, calls, s)"""
    decs = [hip.MLPDecoder(2, 2, 1, 1, 12) for _ in titles]
    planar = (ctypes.POINTER(ctypes.c_int32) * 6)()
    nch = ctypes.c_uint()
    feed = [(d._h, p.ctypes.data, len(p)) for k in range(max(len(t) for t in titles))
            for d, t in zip(decs, titles) for p in [t[k] if k < len(t) else None] if p is not None]
    got = 0
    t0 = time.perf_counter()
    for h, ptr, n in feed:
        got += L.dvda_hip_mlpdecoder_decode_packet(h, ptr, n, planar, ctypes.byref(nch))
    dt = time.perf_counter() - t0
    for d in decs:
        d.close()
    return got, len(feed), dt


def grouped(titles):
    """every title through one member of one group, a call per row of packets -> (PCM frames, group calls, s, steps)"""
    n = len(titles)
    g = hip.MLPDecoderGroup(n)
    frames = (ctypes.c_uint * n)()
    planar = (ctypes.POINTER(ctypes.c_int32) * (6 * n))()
    nch = (ctypes.c_uint * n)()
    rows = []
    for k in range(max(len(t) for t in titles)):
        data, size = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()
        for i, t in enumerate(titles):
            if k < len(t):
                data[i], size[i] = t[k].ctypes.data, len(t[k])
        rows.append((data, size))
    got = 0
    t0 = time.perf_counter()
    for data, size in rows:
        got += L.dvda_hip_mlpdecoder_group_decode_packets(g._h, data, size, frames, planar, nch)
    dt = time.perf_counter() - t0
    steps = g.steps
    g.close()
    return got, len(rows), dt, steps


if not args.group:
    pieces, frames = pieces_of(5)
    for rep in range(max(args.reps, 1)):
        got, calls, dt = lone_in_turn([pieces])
        if rep or args.reps < 2:
            print("tier B%s: %d PCM frames of %d in %d calls, %.3f ms per call, %.2f Msamples/s" % (
                what, got, frames, calls, dt / calls * 1e3, got * 6 / dt / 1e6))
else:
    made = [pieces_of(5 + i) for i in range(args.group)]
    titles, frames = [m[0] for m in made], sum(m[1] for m in made)
    for rep in range(max(args.reps, 1)):
        got, calls, dt, steps = grouped(titles)
        if args.group_only:
            if rep or args.reps < 2:
                print("tier B%s group of %d: %d PCM frames of %d in %d group calls (%d steps), %.3f ms per group call, "
                      "%.2f Msamples/s" % (what, args.group, got, frames, calls, steps, dt / calls * 1e3, got * 6 / dt / 1e6))
            continue
        lgot, lcalls, ldt = lone_in_turn(titles)
        if rep or args.reps < 2:
            print("tier B%s group of %d: %d PCM frames of %d in %d group calls (%d steps), %.3f ms per group call, "
                  "%.2f Msamples/s | %d lone decoders in turn: %d PCM frames in %d calls, %.3f ms per call, %.3f ms per "
                  "round of %d, %.2f Msamples/s | group / lone: %.2fx" % (
                      what, args.group, got, frames, calls, steps, dt / calls * 1e3, got * 6 / dt / 1e6, args.group, lgot,
                      lcalls, ldt / lcalls * 1e3, ldt / calls * 1e3, args.group, lgot * 6 / ldt / 1e6,
                      (got / dt) / (lgot / ldt)))
