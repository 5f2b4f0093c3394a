"""Loader for the CPU oracle (oracle/libmlp_oracle.so) and, when it has been built in
the dev container, the compiled reference (oracle/_ref/libdvda_ref.so).

TEST INFRASTRUCTURE: only tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg import this.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "libmlp_oracle.so")
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libdvda_ref.so")
REF_DIGESTS = os.path.join(ROOT, "tests", "golden", "reference_digests.json")

CHANNELS = [1, 2, 3, 4, 3, 4, 5, 3, 4, 5, 4, 5, 6, 4, 5, 4, 5, 6, 5, 5, 6]


def build_oracle():
    src = os.path.join(ORACLE_DIR, "mlp_oracle.c")
    if (not os.path.exists(ORACLE_SO)) or os.path.getmtime(src) > os.path.getmtime(ORACLE_SO):
        subprocess.run(["make", "-C", ORACLE_DIR, "libmlp_oracle.so"], check=True,
                       stdout=subprocess.DEVNULL)
    return ORACLE_SO


class Stats(ctypes.Structure):
    """mlp_oracle_stats (oracle/mlp_oracle.h): peaks taken in 64 bits before any narrowing, and how often each
    parameter value was read"""
    _fields_ = [("peak_filter_acc", ctypes.c_uint64), ("peak_matrix_acc", ctypes.c_uint64),
                ("peak_sum", ctypes.c_uint64), ("peak_output", ctypes.c_uint64),
                ("value_min", ctypes.c_int64), ("value_max", ctypes.c_int64),
                ("output_shift", ctypes.c_uint32 * 8), ("qss", ctypes.c_uint32 * 16),
                ("noise_shift", ctypes.c_uint32 * 16), ("matrix_frac", ctypes.c_uint32 * 15),
                ("fir_shift", ctypes.c_uint32 * 16), ("iir_shift", ctypes.c_uint32 * 16),
                ("fir_coeff_shift", ctypes.c_uint32 * 8), ("iir_coeff_shift", ctypes.c_uint32 * 8),
                ("fir_order", ctypes.c_uint32 * 9), ("iir_order", ctypes.c_uint32 * 9),
                ("state_bits", ctypes.c_uint32 * 16), ("state_shift", ctypes.c_uint32 * 16),
                ("split8", ctypes.c_uint32 * 9),
                ("fir_min_rail", ctypes.c_uint32), ("fir_max_rail", ctypes.c_uint32),
                ("iir_min_rail", ctypes.c_uint32), ("iir_max_rail", ctypes.c_uint32),
                ("matrix_min_rail", ctypes.c_uint32), ("matrix_max_rail", ctypes.c_uint32),
                ("lsbs_with_book", ctypes.c_uint32 * 25),
                ("offset_min", ctypes.c_int32), ("offset_max", ctypes.c_int32),
                ("state_top_bit_max", ctypes.c_uint32), ("shift_plus_qss_max", ctypes.c_uint32)]


class Oracle:
    def __init__(self):
        self.lib = ctypes.CDLL(build_oracle())
        self.lib.mlp_oracle_decode.restype = ctypes.c_long
        self.lib.mlp_oracle_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                               ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_uint)]
        self.lib.mlp_oracle_decode_stats.restype = ctypes.c_long
        self.lib.mlp_oracle_decode_stats.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                     ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                                     ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(Stats)]

    def decode(self, data, nch, max_frames, chunk=0):
        """-> (pcm int32 [nch, frames], frames, status)"""
        data = np.ascontiguousarray(data, np.uint8)
        cap = int(max_frames) + 16
        out = np.zeros((nch, cap), np.int32)
        st = ctypes.c_uint()
        r = self.lib.mlp_oracle_decode(data.ctypes.data, len(data), chunk, nch, out.ctypes.data, cap,
                                       ctypes.byref(st))
        if r < 0:
            raise RuntimeError("oracle output capacity too small")
        return out[:, :r].copy(), int(r), int(st.value)

    def decode_stats(self, data, nch, max_frames, chunk=0, stats=None):
        """decode() that also adds the decode's statistics to `stats` (a fresh Stats when None)
        -> (pcm, frames, status, stats)"""
        data = np.ascontiguousarray(data, np.uint8)
        cap = int(max_frames) + 16
        out = np.zeros((nch, cap), np.int32)
        st = ctypes.c_uint()
        stats = Stats() if stats is None else stats
        r = self.lib.mlp_oracle_decode_stats(data.ctypes.data, len(data), chunk, nch, out.ctypes.data, cap,
                                             ctypes.byref(st), ctypes.byref(stats))
        if r < 0:
            raise RuntimeError("oracle output capacity too small")
        return out[:, :r].copy(), int(r), int(st.value), stats

    def wav_pack(self, planar, bits):
        """planar int32 [channels, frames] -> the WAV payload bytes dvda2wav writes (oracle/pcm_oracle.c)"""
        planar = np.ascontiguousarray(planar, np.int32)
        ch, frames = planar.shape
        self.lib.wav_oracle_pack.restype = ctypes.c_long
        self.lib.wav_oracle_pack.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_size_t,
                                             ctypes.c_uint, ctypes.c_void_p]
        out = np.zeros(ch * frames * 3 + 8, np.uint8)
        n = self.lib.wav_oracle_pack(planar.ctypes.data, frames, ch, frames, bits, out.ctypes.data)
        return out[:n].tobytes()


class Reference:
    """The real reference decoder; exists only where oracle/_ref has been built."""

    @staticmethod
    def available():
        return os.path.exists(REF_SO)

    def __init__(self):
        self.lib = ctypes.CDLL(REF_SO)
        self.lib.ref_mlp_decode.restype = ctypes.c_long
        self.lib.ref_mlp_decode.argtypes = ([ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t] +
                                            [ctypes.c_uint] * 6 + [ctypes.c_void_p, ctypes.c_size_t])

    def decode(self, data, assignment, rate_code, bps_code, max_frames, chunk=0):
        data = np.ascontiguousarray(data, np.uint8)
        nch = CHANNELS[assignment]
        cap = int(max_frames) + 16
        out = np.zeros((nch, cap), np.int32)
        r = self.lib.ref_mlp_decode(data.ctypes.data, len(data), chunk, bps_code, bps_code, rate_code,
                                    rate_code, assignment, nch, out.ctypes.data, cap)
        if r < 0:
            raise RuntimeError("reference output capacity too small")
        return out[:, :r].copy(), int(r)


def _digest(values):
    h = hashlib.sha256()
    for v in values:
        a = np.ascontiguousarray(v)
        h.update(("%s%s;" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def same_as_reference(key, got, reference_output):
    """True when `got` (a tuple of arrays / numbers) equals what the compiled reference returns for the same input.
    Where oracle/_ref has been built, reference_output() runs the reference and the digest of its result must also be
    the one stored under `key` in tests/golden/reference_digests.json (DVDA_RECORD_REFERENCE=1 stores it instead);
    elsewhere that stored digest stands in for the reference."""
    table = json.load(open(REF_DIGESTS)) if os.path.exists(REF_DIGESTS) else {}
    if Reference.available():
        want = reference_output()
        if os.environ.get("DVDA_RECORD_REFERENCE") == "1":
            table[key] = _digest(want)
            with open(REF_DIGESTS, "w") as f:
                json.dump(table, f, indent=0, sort_keys=True)
                f.write("\n")
        assert table.get(key) == _digest(want), "stored reference digest of %s is missing or stale" % key
        return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert key in table, "no stored reference digest for %s" % key
    return _digest(got) == table[key]
