#!/usr/bin/env python3
"""The decimator's tap tables (libdvd-audio_amd/csrc/pcm_decim_taps.h), from their recipe.

    h = 2 fc sinc(2 fc n) * kaiser(N, 12.0),  fc = 0.5 / D cycles per input sample,  N = 96 D - 1
    normalised to sum 1, rint(h * 2^30), the difference of the sum from 2^30 added to the centre tap

The library's truth is the committed integers, not this recipe: a libm may round a tap the other way, and
tests/test_decimate_model.py allows this tool +-1 per tap against the committed table.

    python tools/make_decim_taps.py            the header's text on stdout
    python tools/make_decim_taps.py --stats    sum, sum of magnitudes, passband ripple and stopband of each table
"""
import sys

import numpy as np

Q = 30
BETA = 12.0
RATIOS = (2, 4)


def length(ratio):
    return 96 * ratio - 1


def make(ratio):
    """-> the N integer taps of `ratio` as a list of Python ints"""
    n_taps = length(ratio)
    half = (n_taps - 1) // 2
    fc = 0.5 / ratio
    n = np.arange(n_taps, dtype=np.float64) - half
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(n_taps, BETA)
    h /= h.sum()
    q = [int(v) for v in np.rint(h * float(1 << Q))]
    q[half] += (1 << Q) - sum(q)
    return q


def response_db(taps, ratio, points=1 << 16):
    """-> (frequencies in units of fs_out, gain in dB) of the integer table, from an FFT of it"""
    h = np.array(taps, np.float64) / float(1 << Q)
    mag = np.abs(np.fft.rfft(h, 2 * points))
    f = np.arange(points + 1) / (2.0 * points) * ratio      # cycles per OUTPUT sample; input Nyquist = ratio / 2
    return f, 20.0 * np.log10(np.maximum(mag, 1e-300))


def stats(taps, ratio):
    f, db = response_db(taps, ratio)
    return dict(sum=sum(taps), sum_abs=sum(abs(v) for v in taps), pass_db=float(np.abs(db[f <= 0.4535]).max()),
                stop_db=float(db[f >= 0.5465].max()))


def header_text():
    out = ["// pcm_decim_taps.h -- the decimator's tap tables (include/dvda_mlp_hip.h states what they are).  Written by",
           "// tools/make_decim_taps.py; these integers, not the recipe, are what the library computes with.",
           "#pragma once", "#include <stdint.h>", "", "namespace dcm {", "", "template <uint32_t D>", "struct Taps;"]
    for d in RATIOS:
        t = make(d)
        out += ["", "template <>", "struct Taps<%du> {" % d, "    static constexpr int32_t h[%d] = {" % len(t)]
        for i in range(0, len(t), 10):
            out.append("        " + " ".join("%d," % v for v in t[i:i + 10]))
        out += ["    };", "};"]
    out += ["", "} // namespace dcm", ""]
    return "\n".join(out)


if __name__ == "__main__":
    if "--stats" in sys.argv[1:]:
        for d in RATIOS:
            print(d, stats(make(d), d))
    else:
        sys.stdout.write(header_text())
