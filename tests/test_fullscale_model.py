"""The generator's two extended modes (libdvd-audio_amd/synth/mlp_synth.h): FULLSCALE -- signal at the scale the format
allows -- and WIDEPARAMS -- every parameter field over the range the reference's parser reads.  TABLE below is the one
list of streams of these modes that the suite decodes: tests/test_gpu_fullscale.py runs the HIP path on exactly these
batches, and the CPU tests here say what the batches are worth:

  envelope   every stream decodes in the restatement with status 0 and its unwrapped values (oracle/mlp_oracle.h,
             mlp_oracle_stats: peak_sum, peak_output) stay below 2^31 -- the generator promises that by bookkeeping
  reach      every FULLSCALE batch reaches the high accumulator word: REACH below
  rails      across the table each extreme of each parameter field occurs: test_rails
  reference  the restatement's PCM is the compiled reference's on every stream (tests/golden/reference_digests.json)

Measured on the table as it stands (log2 of the peak; per FULLSCALE batch, smallest .. largest over the batches):
  |filter accumulator| 36.8 (duo_ss0_4) .. 41.4    |matrix accumulator| 38.9 .. 41.9
  filtered value       most negative -2^24.0 (duo_ss0_4) .. -2^27.2, most positive 2^24.1 .. 2^27.2
REACH asks every batch for 2^36 in both accumulators -- past the low dword and well past the 2^34 the older fuzz streams
reach -- and +-2^22.5 in the filtered value, or for one bit under the smallest figure above where that is more.
Counts over the whole table, per value of the field from its lowest to its highest (test_rails asserts >= 1 of each):
  output_shift 0..7          1138 807 915 234 218 165 138 186
  quant_step_size 0..15      573 232 218 194 190 191 169 194 198 174 176 191 192 233 183 436
  noise_shift 0..15          167 73 99 54 49 48 56 30 38 46 41 53 52 53 51 167
  matrix fractional bits     359 135 151 117 109 140 151 140 161 135 133 167 136 156 1101 (0..14)
  FIR shift 0..15            358 152 138 190 136 167 140 128 163 184 181 153 148 162 180 667
  IIR shift 0..15            166 115 106 158 111 105 116 101 138 111 124 117 132 130 127 456
  FIR / IIR coeff_shift 0..7 2501 236 98 76 61 82 61 132 / 1773 151 88 66 59 47 50 79
  IIR order 0..8             522 390 329 291 275 232 184 210 402
  state_bits 1..15           380 141 115 137 121 115 117 131 119 118 106 125 127 123 338
  state_shift 0..15          320 121 118 119 134 106 115 101 86 139 127 105 107 127 106 382; largest state bit 29 (14 + 15)
  blocks filtered with FIR order k and IIR order 8 - k, k = 0..8: 1443 408 270 338 333 342 357 375 925
  -32768 / +32767: FIR 75 / 60, IIR 36 / 35, matrix 265 / 301       huffman_offset -16384 and 16383 both read
  huffman_lsbs 24 with a code book: 65 channels
  filter shift + quant_step_size on a channel with taps: 30.  Both fields are 4 bits wide (reference src/mlp.c:932,
  1040), so 15 + 15 is the most the syntax carries: the folded shift of csrc/mlp_decode.h is never asked for more.
"""
import hashlib
import math

import numpy as np
import pytest

from tests import oracle_lib
from tests import presentation_model as pm

FULL, WIDE = "FULLSCALE", "WIDEPARAMS"
BOTH = FULL + "|" + WIDE


def _six(features, S, base, **kw):
    """six seeds: assignments 12 and 1, rates 0 / 1 / 2, 24 access units"""
    return [(dict(assignment=12 if i % 2 == 0 else 1, rate_code=i % 3, n_substreams=S, n_aus=24, features=features,
                  restart_interval=[8, 3, 5, 4, 6, 2][i], **kw), base + i) for i in range(6)]


def _four(features, S, base):
    return _six(features, S, base)[:4]


# batch name -> [(generator configuration, seed)]; "features" names the bits ("SF_FAST" / "SF_ALL": the sets of synth.py)
TABLE = {}
for _S in (1, 2):
    # lane kernels and cooperative kernel
    TABLE["full_S%d" % _S] = _six(FULL, _S, 61000 + 100 * _S)
    TABLE["wide_S%d" % _S] = _six(WIDE, _S, 62000 + 100 * _S)
    TABLE["both_fast_S%d" % _S] = _six(BOTH + "|SF_FAST", _S, 63000 + 100 * _S)
    # chain passes
    TABLE["chained_firrand_S%d" % _S] = _four(BOTH + "|CHAINED|FIRRAND", _S, 64000 + 100 * _S)
    TABLE["disc_chained_mixbooks_S%d" % _S] = _four(BOTH + "|DISC|CHAINED|MIXBOOKS", _S, 65000 + 100 * _S)
    TABLE["iir_S%d" % _S] = _four(BOTH + "|IIR", _S, 66000 + 100 * _S)
    # sequential and general pass
    TABLE["midrestart_varblock_S%d" % _S] = _four(BOTH + "|MIDRESTART|VARBLOCK", _S, 67000 + 100 * _S)
    TABLE["midmatrix_S%d" % _S] = _four(BOTH + "|MIDMATRIX|PARAMBLOCKS|MATRIXRAND|QSS|OUTSHIFT", _S, 68000 + 100 * _S)
    TABLE["varrows_S%d" % _S] = _four(BOTH + "|VARROWS", _S, 69000 + 100 * _S)
# two substreams, every split of six channels
for _k in range(1, 6):
    TABLE["duo_ss0_%d" % _k] = [
        (dict(assignment=12, rate_code=1, n_substreams=2, n_aus=24, ss0_channels=_k, features=BOTH + "|SF_FAST",
              restart_interval=5), 70000 + 10 * _k),
        (dict(assignment=12, rate_code=1, n_substreams=2, n_aus=24, ss0_channels=_k, features=BOTH + "|CHAINED",
              restart_interval=4), 70001 + 10 * _k)]
# lanes of one wave that disagree: odd titles at full scale with wide parameters, even titles the plain recipe
TABLE["disagree_128"] = [(dict(assignment=12, rate_code=1, n_substreams=1, n_aus=8, features=BOTH if i & 1 else "",
                               restart_interval=4), 71000 + i) for i in range(128)]
# streaming tier
TABLE["streaming"] = [
    (dict(assignment=12, rate_code=1, n_substreams=2, n_aus=24, features=BOTH, restart_interval=4), 72000),
    (dict(assignment=1, rate_code=0, n_substreams=1, n_aus=24, features=BOTH + "|CHAINED", restart_interval=5), 72001),
    (dict(assignment=12, rate_code=2, n_substreams=1, n_aus=24, features=BOTH + "|SF_FAST", restart_interval=3), 72002)]
# the presentation of substream 0 (decoded on its own: its matrices and output shifts apply there and only there)
TABLE["presentation"] = [(dict(assignment=12, rate_code=1, n_substreams=2, n_aus=24, ss0_channels=[2, 2, 1, 3][i],
                               features=[BOTH, BOTH + "|CHAINED", BOTH + "|SF_FAST", BOTH + "|DISC|CHAINED"][i],
                               restart_interval=[8, 4, 5, 8][i]), 73000 + i) for i in range(4)]

# log2 of |filter accumulator|, |matrix accumulator|, |filtered value| of either sign that every FULLSCALE batch reaches:
# 36 / 36 / 22.5, or one bit under the smallest peak over the batches (module docstring) where that is more
REACH = (36.0, 37.9, 23.0)


def feature_bits(syn, text):
    bits = 0
    for name in filter(None, text.split("|")):
        bits |= {"SF_FAST": syn.SF_FAST, "SF_ALL": syn.SF_ALL}.get(name) or syn.SF[name]
    return bits


def is_extended(kw):
    return FULL in kw["features"] or WIDE in kw["features"]


def is_fullscale(name):
    return all(FULL in kw["features"] for kw, _ in TABLE[name] if kw["features"])


def cases(pkg, name):
    """-> [(cfg, seed)] of a batch, the form tests/test_gpu_parity.py's _check takes"""
    syn = pkg.synth
    out = []
    for kw, seed in TABLE[name]:
        kw = dict(kw)
        bits = feature_bits(syn, kw.pop("features"))
        out.append((syn.make_cfg(profile=1 if bits else 0, features=bits, **kw), seed))
    return out


_STREAMS = {}


def streams(pkg, name):
    """-> [(cfg, bytes, PCM frames)] of a batch, generated once"""
    if name not in _STREAMS:
        _STREAMS[name] = [(cfg,) + pkg.synth.stream(cfg, seed) for cfg, seed in cases(pkg, name)]
    return _STREAMS[name]


_DECODED = {}


def decoded(pkg, oracle, name):
    """-> [(pcm, frames, status, Stats)] of a batch from the restatement, decoded once and left unchanged"""
    if name not in _DECODED:
        _DECODED[name] = [oracle.decode_stats(b, pkg.synth.channels(cfg.assignment), f) for cfg, b, f in streams(pkg, name)]
    return _DECODED[name]


def _log2(x):
    return math.log2(x) if x > 0 else float("-inf")


@pytest.mark.parametrize("name", sorted(TABLE))
def test_envelope(pkg, oracle, name):
    for (cfg, b, f), (pcm, r, status, st) in zip(streams(pkg, name), decoded(pkg, oracle, name)):
        assert status == 0 and r == f
        assert st.peak_sum < 1 << 31 and st.peak_output < 1 << 31, (_log2(st.peak_sum), _log2(st.peak_output))
        if name == "presentation":
            # substream 0 on its own is a stream too: the same promise holds for it
            one, k, est = pm.strip(b)
            assert est == 0
            _, r1, status1, st1 = oracle.decode_stats(one, k, f)
            assert status1 == 0 and r1 == f
            assert st1.peak_sum < 1 << 31 and st1.peak_output < 1 << 31


def test_envelope_beyond_the_table(pkg, oracle):
    """the bookkeeping is not tuned to the table's seeds: 120 more streams, other layouts and feature sets among them"""
    syn = pkg.synth
    n = 0
    for text in (FULL, WIDE, BOTH + "|SF_ALL", BOTH + "|DISC|CHAINED|SYNCONLY", BOTH + "|FLAGS|MIDRESTART|NOCHECK"):
        for asg, S in ((12, 1), (0x14, 2), (0, 1), (6, 2)):
            for seed in range(6):
                cfg = syn.make_cfg(assignment=asg, rate_code=[0, 1, 2, 9, 8, 10][seed], n_substreams=S, n_aus=12, profile=1,
                                   features=feature_bits(syn, text), restart_interval=[4, 1, 3, 12, 2, 5][seed])
                b, f = syn.stream(cfg, 80000 + n)
                _, r, status, st = oracle.decode_stats(b, syn.channels(asg), f)
                assert status == 0 and r == f, (text, asg, S, seed, hex(status))
                assert st.peak_sum < 1 << 31 and st.peak_output < 1 << 31, (text, asg, S, seed)
                n += 1
    assert n == 120


@pytest.mark.parametrize("name", sorted(n for n in TABLE if is_fullscale(n)))
def test_reach(pkg, oracle, name):
    stats = [st for _, _, _, st in decoded(pkg, oracle, name)]
    got = (_log2(max(s.peak_filter_acc for s in stats)), _log2(max(s.peak_matrix_acc for s in stats)),
           _log2(-min(s.value_min for s in stats)), _log2(max(s.value_max for s in stats)))
    print("%s: filter acc 2^%.1f matrix acc 2^%.1f value -2^%.1f .. 2^%.1f" % ((name,) + got))
    assert got[0] >= REACH[0] and got[1] >= REACH[1] and got[2] >= REACH[2] and got[3] >= REACH[2]


def test_rails(pkg, oracle):
    """each end of each field of the two modes occurs in the table (counts: module docstring)"""
    tot = oracle_lib.Stats()
    arrays = [n for n, t in oracle_lib.Stats._fields_ if hasattr(t, "_length_")]
    scalars = ["fir_min_rail", "fir_max_rail", "iir_min_rail", "iir_max_rail", "matrix_min_rail", "matrix_max_rail"]
    for name in sorted(TABLE):
        for (kw, _), (_, _, _, st) in zip(TABLE[name], decoded(pkg, oracle, name)):
            if not is_extended(kw):
                continue
            for n in arrays:
                a, b = getattr(tot, n), getattr(st, n)
                for i in range(len(a)):
                    a[i] += b[i]
            for n in scalars:
                setattr(tot, n, getattr(tot, n) + getattr(st, n))
            tot.offset_min = min(tot.offset_min, st.offset_min)
            tot.offset_max = max(tot.offset_max, st.offset_max)
            tot.state_top_bit_max = max(tot.state_top_bit_max, st.state_top_bit_max)
            tot.shift_plus_qss_max = max(tot.shift_plus_qss_max, st.shift_plus_qss_max)
    for n in arrays:
        print(n, list(getattr(tot, n)))
    print({n: getattr(tot, n) for n in scalars}, tot.offset_min, tot.offset_max, tot.state_top_bit_max,
          tot.shift_plus_qss_max)
    for n, hi in (("output_shift", 7), ("qss", 15), ("noise_shift", 15), ("matrix_frac", 14), ("fir_shift", 15),
                  ("iir_shift", 15), ("fir_coeff_shift", 7), ("iir_coeff_shift", 7), ("state_shift", 15)):
        a = getattr(tot, n)
        assert a[0] >= 1 and a[hi] >= 1, n
        assert all(a[i] >= 1 for i in range(hi + 1)), n         # ... and everything between
    assert tot.state_bits[1] >= 1 and tot.state_bits[15] >= 1 and tot.state_bits[0] == 0
    assert tot.state_top_bit_max == 29                          # 14 + 15: the state still fits int32
    assert (tot.offset_min, tot.offset_max) == (-16384, 16383)
    assert tot.iir_order[8] >= 1 and tot.fir_order[8] >= 1
    assert all(tot.split8[k] >= 1 for k in range(9))            # every split of 8 taps, IIR order 8 with no FIR among them
    assert all(getattr(tot, n) >= 1 for n in scalars)           # -32768 and +32767 in FIR, IIR and matrix
    assert tot.lsbs_with_book[24] >= 1
    assert tot.shift_plus_qss_max == 30                         # 15 + 15 on a channel with taps (see the docstring)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_equals_the_compiled_reference(pkg, oracle, name):
    for i, ((kw, seed), (cfg, b, f), (pcm, r, status, _)) in enumerate(
            zip(TABLE[name], streams(pkg, name), decoded(pkg, oracle, name))):
        if not is_extended(kw):
            continue
        assert status == 0
        assert oracle_lib.same_as_reference(
            "fullscale_%s_%d" % (name, i), (pcm, r),
            lambda: oracle_lib.Reference().decode(b, cfg.assignment, cfg.rate_code, cfg.bps_code, f))


def test_the_two_bits_stay_out_of_the_all_features_set(pkg):
    syn = pkg.synth
    assert syn.SF["FULLSCALE"] == 1 << 21 and syn.SF["WIDEPARAMS"] == 1 << 22
    assert syn.SF_ALL & (syn.SF["FULLSCALE"] | syn.SF["WIDEPARAMS"]) == 0
    # ... and mean nothing to the recipe
    a, _ = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_aus=8), 5)
    b, _ = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_aus=8, features=syn.SF["FULLSCALE"] | syn.SF["WIDEPARAMS"]), 5)
    assert np.array_equal(a, b)


def test_streams_of_the_old_features_are_what_they_were(pkg):
    """SHA-256 of three streams as the generator made them before the two bits existed"""
    syn = pkg.synth
    SF = syn.SF
    for cfg, seed, size, want in (
            (syn.make_cfg(assignment=12, rate_code=1, n_aus=32), 1, 31268,
             "8c1167a92dbeb8db36c6da28dd777f4a8d83b50d5e443fad93a3e62e116e6c2a"),
            (syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=32, profile=1, features=syn.SF_ALL,
                          restart_interval=5), 2, 26528,
             "d4a30322c87e2634ae61657c713cef3a8b079df5f0972d1e8aacff2c633bdbbf"),
            (syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=32, profile=1,
                          features=SF["DISC"] | SF["CHAINED"] | SF["FIRRAND"] | SF["MIXBOOKS"], restart_interval=8), 3, 21984,
             "7bc9364bc867de7263a865c3cf5667b61778b02f25d796f366f28c111984506c")):
        b, _ = syn.stream(cfg, seed)
        assert len(b) == size and hashlib.sha256(b.tobytes()).hexdigest() == want
