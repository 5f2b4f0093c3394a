#!/usr/bin/env python3
"""The resampler's tap table (libdvd-audio_amd/csrc/pcm_resample_taps.h), from its recipe.

    h_c(t) = (147/160) sinc((147/160) t) * I0(12 sqrt(1 - (t/48)^2)) / I0(12),  t in input samples
    g[p][i] = h_c(i - 47 - p/147),  p = 0 .. 146,  i = 0 .. 95
    every phase normalised to sum 1, rint(g * 2^30), the difference of the phase's sum from 2^30 added to the phase's
    largest tap

The library's truth is the committed integers, not this recipe: a libm may round a tap the other way, and
tests/test_resample_model.py allows this tool +-1 per tap against the committed table.

    python tools/make_resample_taps.py            the header's text on stdout
    python tools/make_resample_taps.py --stats    sums, sum of magnitudes, passband ripple and stopband of the table
"""
import sys

import numpy as np

Q = 30
BETA = 12.0
L, M = 147, 160                 # 48 000 Hz * L / M = 44 100 Hz
TAPS = 96
FRONT = 47                      # input frames of a window in front of frame q; TAPS - 1 - FRONT = 48 behind it
HALF = 48.0                     # the window's half width in input samples


def prototype(t):
    """h_c at the times t (input samples)"""
    t = np.asarray(t, np.float64)
    w = np.i0(BETA * np.sqrt(np.maximum(1.0 - (t / HALF) ** 2, 0.0))) / np.i0(BETA)
    return (L / M) * np.sinc((L / M) * t) * np.where(np.abs(t) <= HALF, w, 0.0)


def make():
    """-> the table as a list of L lists of TAPS Python ints"""
    table = []
    for p in range(L):
        g = prototype(np.arange(TAPS, dtype=np.float64) - FRONT - p / float(L))
        g /= g.sum()
        q = [int(v) for v in np.rint(g * float(1 << Q))]
        q[int(np.argmax(q))] += (1 << Q) - sum(q)
        table.append(q)
    return table


def response_db(table, points=1 << 20):
    """-> (frequencies in units of fs_out, gain in dB) of the integer table: an FFT of the whole L-times oversampled
    prototype the phases are cut from, images included"""
    g = np.asarray(table, np.float64) / float(1 << Q)
    proto = np.zeros(L * (TAPS + 1))
    for p in range(L):
        for i in range(TAPS):
            proto[L * (i + 1) - p] = g[p][i]            # time (i - 47 - p / L) input samples, shifted to be >= 0
    mag = np.abs(np.fft.rfft(proto, 2 * points)) / L
    f = np.arange(points + 1) / (2.0 * points) * M      # cycles per OUTPUT sample: the prototype runs at M fs_out
    return f, 20.0 * np.log10(np.maximum(mag, 1e-300))


def stats(table):
    f, db = response_db(table)
    return dict(sums=sorted(set(sum(r) for r in table)), max_sum_abs=max(sum(abs(v) for v in r) for r in table),
                pass_hi_db=float(db[f <= 0.4535].max()), pass_lo_db=float(db[f <= 0.4535].min()),
                stop_db=float(db[f >= 0.5465].max()))


def header_text():
    out = ["// pcm_resample_taps.h -- the resampler's tap table g[147][96] (include/dvda_mlp_hip.h states what it is).  Written",
           "// by tools/make_resample_taps.py; these integers, not the recipe, are what the library computes with.",
           "#pragma once", "#include <stdint.h>", "", "namespace rsm {", "",
           "constexpr uint32_t PHASES = %du, TAPS = %du;" % (L, TAPS), "",
           "struct Table {", "    static constexpr int32_t g[PHASES][TAPS] = {"]
    for p, row in enumerate(make()):
        out.append("        { // phase %d" % p)
        for i in range(0, TAPS, 8):
            out.append("            " + " ".join("%d," % v for v in row[i:i + 8]))
        out.append("        },")
    out += ["    };", "};", "", "} // namespace rsm", ""]
    return "\n".join(out)


if __name__ == "__main__":
    if "--stats" in sys.argv[1:]:
        print(stats(make()))
    else:
        sys.stdout.write(header_text())
