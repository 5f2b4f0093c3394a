"""ctypes binding of the C ABI in include/dvda_mlp_hip.h (batch tier).

torch is used for what it is good at here -- device memory and streams; every
compute step is the HIP library.  There is no CPU fallback: a missing library,
a missing GPU or a HIP error raises.
"""
import contextlib
import ctypes

import numpy as np

from . import _build

ST = dict(NO_SYNC=1 << 0, SYNC_CHANGE=1 << 1, PARITY=1 << 2, CRC=1 << 3, EOF=1 << 4, RESTART=1 << 5,
          PARAMS=1 << 6, HUFFMAN=1 << 7, FILTER=1 << 8, ENVELOPE=1 << 9, IRREGULAR=1 << 16,
          TIMING=1 << 17, MIDFRAME=1 << 18, CHAINED=1 << 19, OVERFLOW=1 << 20, TRUNCATED=1 << 21,
          CAPACITY=1 << 22, GENERAL=1 << 23, FALSE_SYNC=1 << 24, SEQ=1 << 25, COLD=1 << 26, YIELD=1 << 27)
# bits that do not invalidate the decoded PCM: the conditions the fast pass defers are informational
# once the passes behind it have decoded them (any failure there sets an error bit); a dropped
# access unit (later major sync with other stream parameters) is what the reference does too
ST_BENIGN = (ST["TRUNCATED"] | ST["CHAINED"] | ST["MIDFRAME"] | ST["TIMING"] | ST["GENERAL"] | ST["SEQ"] |
             ST["SYNC_CHANGE"] | ST["COLD"] | ST["YIELD"])


class StreamInfo(ctypes.Structure):
    _fields_ = [("mlp_frames", ctypes.c_uint64), ("pcm_frames", ctypes.c_uint64),
                ("bytes_consumed", ctypes.c_uint64), ("status", ctypes.c_uint32),
                ("channels", ctypes.c_uint32), ("substreams", ctypes.c_uint32),
                ("assignment", ctypes.c_uint32), ("group0_bps", ctypes.c_uint32),
                ("group1_bps", ctypes.c_uint32), ("group0_rate", ctypes.c_uint32),
                ("group1_rate", ctypes.c_uint32), ("segments", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class SegmentInfo(ctypes.Structure):
    """dvda_mlp_segment_info of include/dvda_mlp_hip.h"""
    _fields_ = [("offset", ctypes.c_uint64), ("end", ctypes.c_uint64), ("stream", ctypes.c_uint32),
                ("mlp_frames", ctypes.c_uint32), ("pcm_frames", ctypes.c_uint32), ("status", ctypes.c_uint32)]


class MultiSummary(ctypes.Structure):
    """dvda_mlp_multi_summary of include/dvda_mlp_hip.h"""
    _fields_ = [("pcm_frames", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("compressed_bytes", ctypes.c_uint64),
                ("compressed_bytes_max_device", ctypes.c_uint64), ("streams_with_errors", ctypes.c_uint32),
                ("devices", ctypes.c_uint32), ("device_ms_max", ctypes.c_double), ("device_ms_min", ctypes.c_double),
                ("imbalance", ctypes.c_double), ("reduction", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HipError(RuntimeError):
    pass


_lib = None

EXPORTS = ("dvda_mlp_hip_create", "dvda_mlp_hip_destroy", "dvda_mlp_hip_index", "dvda_mlp_hip_decode",
           "dvda_mlp_hip_stream_info", "dvda_mlp_hip_segment_count", "dvda_mlp_hip_kernel_time",
           "dvda_mlp_hip_version", "dvda_mlp_hip_selftest_huff", "dvda_mlp_hip_selftest_bits",
           "dvda_mlp_hip_bounds_violations", "dvda_mlp_hip_decode_async", "dvda_mlp_hip_reserve",
           "dvda_mlp_hip_decode_time",
           "dvda_mlp_hip_set_lanes_per_segment", "dvda_mlp_hip_set_chain_form",
           "dvda_mlp_hip_set_pcm_layout", "dvda_mlp_hip_segment_info",
           "dvda_mlp_hip_segment_fir", "dvda_mlp_hip_set_initial_fir",
           "dvda_hip_open_mlpdecoder", "dvda_hip_close_mlpdecoder", "dvda_hip_mlpdecoder_decode_packet",
           "dvda_hip_mlpdecoder_status", "dvda_hip_mlpdecoder_queued_bytes", "dvda_hip_mlpdecoder_path",
           "dvda_hip_open_mlpdecoder_group", "dvda_hip_close_mlpdecoder_group", "dvda_hip_mlpdecoder_group_size",
           "dvda_hip_mlpdecoder_group_decode_packets", "dvda_hip_mlpdecoder_group_status",
           "dvda_hip_mlpdecoder_group_queued_bytes", "dvda_hip_mlpdecoder_group_path", "dvda_hip_mlpdecoder_group_steps",
           "dvda_pcm_hip_workspace_words", "dvda_pcm_hip_decode_sectors", "dvda_pcm_hip_result",
           "dvda_mlp_hip_demux_sectors", "dvda_mlp_hip_pack_wav",
           "dvda_mlp_hip_shard", "dvda_mlp_hip_create_multi", "dvda_mlp_hip_destroy_multi",
           "dvda_mlp_hip_multi_devices", "dvda_mlp_hip_decode_multi", "dvda_mlp_hip_multi_device_time",
           "dvda_mlp_hip_set_conceal", "dvda_mlp_hip_conceal_spans", "dvda_mlp_hip_conceal_edges",
           "dvda_mlp_hip_set_presentation", "dvda_mlp_hip_present_time", "dvda_mlp_hip_present_read",
           "dvda_pcm_hip_crc32", "dvda_pcm_hip_crc32_workspace_words", "dvda_mlp_hip_pcm_crc32",
           "dvda_pcm_hip_crc32_combine",
           "dvda_pcm_hip_levels", "dvda_pcm_hip_levels_workspace_words", "dvda_mlp_hip_pcm_levels",
           "dvda_pcm_hip_levels_combine",
           "dvda_pcm_hip_compare", "dvda_pcm_hip_compare_workspace_words", "dvda_mlp_hip_pcm_compare",
           "dvda_pcm_hip_diff_combine", "dvda_mlp_hip_index_graph_state",
           "dvda_pcm_hip_energy", "dvda_pcm_hip_energy_workspace_words", "dvda_mlp_hip_pcm_energy",
           "dvda_pcm_hip_energy_append", "dvda_pcm_hip_energy_total",
           "dvda_pcm_hip_requantize", "dvda_pcm_hip_requantize_workspace_words", "dvda_mlp_hip_pcm_requantize",
           "dvda_pcm_hip_requant_value",
           "dvda_pcm_hip_decimate", "dvda_pcm_hip_decimate_workspace_words", "dvda_mlp_hip_pcm_decimate",
           "dvda_pcm_hip_decim_taps", "dvda_pcm_hip_decim_out_frames", "dvda_pcm_hip_decim_value",
           "dvda_pcm_hip_resample", "dvda_pcm_hip_resample_workspace_words", "dvda_mlp_hip_pcm_resample",
           "dvda_pcm_hip_resample_taps", "dvda_pcm_hip_resample_out_frames", "dvda_pcm_hip_resample_value",
           "dvda_pcm_hip_mix", "dvda_pcm_hip_mix_workspace_words", "dvda_mlp_hip_pcm_mix",
           "dvda_pcm_hip_speaker_mask", "dvda_pcm_hip_mix_matrix", "dvda_pcm_hip_mix_valid", "dvda_pcm_hip_mix_value")

CRC_TILE_BYTES = 16384      # DVDA_CRC_TILE_BYTES: the digest's tiles, aligned to the end of a stream's payload
CRC_JOIN_TILES = 256        # DVDA_CRC_JOIN_TILES: tiles a join workgroup folds per turn of its loop


class _Record(ctypes.Structure):
    """A result or parameter struct of include/dvda_mlp_hip.h whose dict form follows from its _fields_: a scalar is an
    int, an array a list of int, a field named `reserved` is left out (and zero on the way back)."""

    def as_dict(self):
        out = {}
        for k, _ in self._fields_:
            if k != "reserved":
                out[k] = _plain(getattr(self, k))
        return out

    @classmethod
    def from_dict(cls, d):
        return cls(**{k: _typed(t, d[k]) for k, t in cls._fields_ if k != "reserved"})


def _plain(v):
    """a field of a record -> int, or (nested) lists of int for an array"""
    return [_plain(e) for e in v] if isinstance(v, ctypes.Array) else int(v)


def _typed(t, v):
    """... and back: the value of ctypes type t"""
    return t(*[_typed(t._type_, e) for e in v]) if issubclass(t, ctypes.Array) else v


class CrcDesc(ctypes.Structure):
    """dvda_pcm_crc_desc of include/dvda_mlp_hip.h"""
    _fields_ = [("off", ctypes.c_uint64), ("stride", ctypes.c_uint64), ("frames", ctypes.c_uint64),
                ("channels", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

LVL_TILE_FRAMES = 4096      # DVDA_LVL_TILE_FRAMES: the level report's tiles, aligned to the start of a stream


class Levels(_Record):
    """dvda_pcm_levels of include/dvda_mlp_hip.h"""
    _fields_ = [("frames", ctypes.c_uint64), ("lead_silent", ctypes.c_uint64), ("trail_silent", ctypes.c_uint64),
                ("sum", ctypes.c_int64 * 8), ("over", ctypes.c_uint64 * 8), ("min", ctypes.c_int32 * 8),
                ("max", ctypes.c_int32 * 8)]


CMP_TILE_FRAMES = 4096      # DVDA_CMP_TILE_FRAMES: the compare's tiles, aligned to the start of a stream pair
CMP_SHAPE = 1               # DVDA_CMP_SHAPE: nothing was compared, the two descriptors do not go together


class Diff(_Record):
    """dvda_pcm_diff of include/dvda_mlp_hip.h"""
    _fields_ = [("frames_a", ctypes.c_uint64), ("frames_b", ctypes.c_uint64), ("compared", ctypes.c_uint64),
                ("diff_frames", ctypes.c_uint64), ("first_diff", ctypes.c_uint64), ("diff_end", ctypes.c_uint64),
                ("runs", ctypes.c_uint64), ("diff_values", ctypes.c_uint64 * 8), ("max_abs", ctypes.c_uint32 * 8),
                ("channels", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


NRG_MIN_BLOCK, NRG_MAX_BLOCK = 64, 1 << 24      # DVDA_NRG_MIN_BLOCK / DVDA_NRG_MAX_BLOCK: the energy report's block length
NRG_PIECE_FRAMES = 4096     # DVDA_NRG_PIECE_FRAMES: frames of one block a workgroup takes at most


class EnergyBlock(_Record):
    """dvda_pcm_energy_block of include/dvda_mlp_hip.h"""
    _fields_ = [("sq_lo", ctypes.c_uint64 * 8), ("sq_hi", ctypes.c_uint64 * 8), ("peak", ctypes.c_uint32 * 8),
                ("frames", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


RQ_TRUNCATE, RQ_ROUND, RQ_TPDF = 0, 1, 2        # DVDA_RQ_*: how the word-length reduction treats the bits it drops


class Requant(_Record):
    """dvda_pcm_requant of include/dvda_mlp_hip.h"""
    _fields_ = [("bits_in", ctypes.c_uint32), ("bits_out", ctypes.c_uint32), ("mode", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("seed", ctypes.c_uint64)]


class RequantReport(_Record):
    """dvda_pcm_requant_report of include/dvda_mlp_hip.h"""
    _fields_ = [("frames", ctypes.c_uint64), ("clipped", ctypes.c_uint64 * 8)]


DCM_TILE_FRAMES = 1024      # DVDA_DCM_TILE_FRAMES: OUTPUT frames of the decimator's tiles, aligned to a stream's first output frame
DECIM_RATES = (44100, 48000, 88200, 96000)      # the rates decode_streams_decimated hands out


RSM_TILE_FRAMES = 9408      # DVDA_RSM_TILE_FRAMES: OUTPUT frames of the resampler's tiles (64 * 147), aligned as the decimator's
RSM_PHASES, RSM_TAPS = 147, 96      # the resampler's table: 48 000 Hz * 147 / 160 = 44 100 Hz
RESAMPLE_RATE = 44100       # the one rate decode_streams_resampled hands out


class DecimPiece(ctypes.Structure):
    """dvda_pcm_decim_piece of include/dvda_mlp_hip.h"""
    _fields_ = [("frame0", ctypes.c_uint64), ("before", ctypes.c_uint32), ("after", ctypes.c_uint32)]


class DecimReport(_Record):
    """dvda_pcm_decim_report of include/dvda_mlp_hip.h"""
    _fields_ = [("frames_in", ctypes.c_uint64), ("frames_out", ctypes.c_uint64), ("clipped", ctypes.c_uint64 * 8)]


MIX_NORMALIZED, MIX_UNITY, MIX_LFE = 0, 1, 2     # DVDA_MIX_*: how dvda_pcm_hip_mix_matrix scales, and whether the LFE takes part


class PcmMix(_Record):
    """dvda_pcm_mix of include/dvda_mlp_hip.h"""
    _fields_ = [("in_channels", ctypes.c_uint32), ("out_channels", ctypes.c_uint32), ("coef", (ctypes.c_int32 * 8) * 8)]


class PcmMixReport(_Record):
    """dvda_pcm_mix_report of include/dvda_mlp_hip.h"""
    _fields_ = [("frames", ctypes.c_uint64), ("clipped", ctypes.c_uint64 * 8)]


ST_CONCEALED = 1 << 30          # DVDA_ST_CONCEALED: conceal mode, the stream was damaged (not in ST_BENIGN)
CONCEAL_LEADING, CONCEAL_TRAILING, CONCEAL_ROUNDS = 1, 2, 4     # DVDA_CONCEAL_* span flags


class ConcealSpan(ctypes.Structure):
    """dvda_mlp_conceal_span of include/dvda_mlp_hip.h"""
    _fields_ = [("first_frame", ctypes.c_uint64), ("frames", ctypes.c_uint64), ("byte_off", ctypes.c_uint64),
                ("byte_end", ctypes.c_uint64), ("cause", ctypes.c_uint32), ("flags", ctypes.c_uint32)]

    def as_tuple(self):
        return (int(self.first_frame), int(self.frames), int(self.byte_off), int(self.byte_end), int(self.cause),
                int(self.flags))


class ConcealEdges(ctypes.Structure):
    """dvda_mlp_conceal_edges of include/dvda_mlp_hip.h"""
    _fields_ = [("kept_begin", ctypes.c_uint64), ("kept_end", ctypes.c_uint64), ("t_first", ctypes.c_uint32),
                ("t_end", ctypes.c_uint32), ("kept_bytes", ctypes.c_uint64), ("kept_frames", ctypes.c_uint64),
                ("ends_kept", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("fir", ctypes.c_int32 * 96)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("kept_begin", "kept_end", "t_first", "t_end", "kept_bytes", "kept_frames",
                                                 "ends_kept")}
        d["fir"] = np.array(self.fir, np.int32).reshape(2, 48)
        return d


def lib():
    """Loads (building if stale) libdvda_mlp_hip.so; raises if it cannot."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64.so.7; import it FIRST so this library
        # binds to the same HIP runtime (two runtimes in one process do not share
        # devices or pointers)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        import os
        so = os.environ.get("DVDA_MLP_HIP_LIB") or _build.build_hip()   # override: diagnostic A/B builds
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.dvda_mlp_hip_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, u32, u32]
        L.dvda_mlp_hip_destroy.argtypes = [vp]
        L.dvda_mlp_hip_destroy.restype = None
        L.dvda_mlp_hip_index.argtypes = [vp, vp, u64, vp, vp, u32, vp]
        L.dvda_mlp_hip_decode.argtypes = [vp, vp, vp, vp, vp]
        L.dvda_mlp_hip_decode_async.argtypes = [vp, vp, vp, vp, vp]
        L.dvda_mlp_hip_reserve.argtypes = [vp, u64, u32, u32]
        L.dvda_mlp_hip_stream_info.argtypes = [vp, ctypes.POINTER(StreamInfo), u32, vp]
        L.dvda_mlp_hip_segment_count.argtypes = [vp, ctypes.POINTER(u32), vp]
        L.dvda_mlp_hip_index_graph_state.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        L.dvda_mlp_hip_kernel_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32)]
        L.dvda_mlp_hip_decode_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32)]
        L.dvda_mlp_hip_set_lanes_per_segment.argtypes = [vp, u32]
        L.dvda_mlp_hip_set_pcm_layout.argtypes = [vp, u32]
        L.dvda_mlp_hip_set_chain_form.argtypes = [vp, u32]
        L.dvda_mlp_hip_version.restype = ctypes.c_char_p
        L.dvda_hip_open_mlpdecoder.restype = vp
        L.dvda_hip_open_mlpdecoder.argtypes = [ctypes.c_uint] * 5 + [ctypes.c_int]
        L.dvda_hip_close_mlpdecoder.argtypes = [vp]
        L.dvda_hip_close_mlpdecoder.restype = None
        L.dvda_hip_mlpdecoder_decode_packet.restype = ctypes.c_uint
        L.dvda_hip_mlpdecoder_decode_packet.argtypes = [vp, vp, ctypes.c_size_t,
                                                        ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)),
                                                        ctypes.POINTER(ctypes.c_uint)]
        L.dvda_hip_mlpdecoder_status.restype = ctypes.c_uint
        L.dvda_hip_mlpdecoder_status.argtypes = [vp]
        L.dvda_hip_mlpdecoder_queued_bytes.restype = ctypes.c_size_t
        L.dvda_hip_mlpdecoder_queued_bytes.argtypes = [vp]
        L.dvda_hip_mlpdecoder_path.argtypes = [vp]
        L.dvda_hip_open_mlpdecoder_group.restype = vp
        L.dvda_hip_open_mlpdecoder_group.argtypes = [ctypes.c_uint, ctypes.c_int]
        L.dvda_hip_close_mlpdecoder_group.argtypes = [vp]
        L.dvda_hip_close_mlpdecoder_group.restype = None
        L.dvda_hip_mlpdecoder_group_size.restype = ctypes.c_uint
        L.dvda_hip_mlpdecoder_group_size.argtypes = [vp]
        L.dvda_hip_mlpdecoder_group_decode_packets.restype = ctypes.c_ulonglong
        L.dvda_hip_mlpdecoder_group_decode_packets.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t),
                                                               ctypes.POINTER(ctypes.c_uint),
                                                               ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)),
                                                               ctypes.POINTER(ctypes.c_uint)]
        L.dvda_hip_mlpdecoder_group_status.restype = ctypes.c_uint
        L.dvda_hip_mlpdecoder_group_status.argtypes = [vp, ctypes.c_uint]
        L.dvda_hip_mlpdecoder_group_queued_bytes.restype = ctypes.c_size_t
        L.dvda_hip_mlpdecoder_group_queued_bytes.argtypes = [vp, ctypes.c_uint]
        L.dvda_hip_mlpdecoder_group_path.argtypes = [vp, ctypes.c_uint]
        L.dvda_hip_mlpdecoder_group_steps.restype = ctypes.c_ulonglong
        L.dvda_hip_mlpdecoder_group_steps.argtypes = [vp]
        L.dvda_pcm_hip_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_workspace_words.argtypes = [u32]
        L.dvda_pcm_hip_decode_sectors.argtypes = [vp, u32, ctypes.c_uint, ctypes.c_uint, vp, u64, vp, vp]
        L.dvda_pcm_hip_result.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u32), vp]
        L.dvda_mlp_hip_demux_sectors.argtypes = [vp, u32, vp, u64, vp, vp]
        L.dvda_mlp_hip_pack_wav.argtypes = [vp, u64, ctypes.c_uint, u64, ctypes.c_uint, vp, vp]
        L.dvda_mlp_hip_shard.argtypes = [vp, u32, u32, vp]
        L.dvda_mlp_hip_create_multi.argtypes = [ctypes.POINTER(vp), vp, u32, u32, u32]
        L.dvda_mlp_hip_destroy_multi.argtypes = [vp]
        L.dvda_mlp_hip_destroy_multi.restype = None
        L.dvda_mlp_hip_multi_devices.argtypes = [vp]
        L.dvda_mlp_hip_multi_devices.restype = u32
        L.dvda_mlp_hip_multi_device_time.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
        L.dvda_mlp_hip_decode_multi.argtypes = [vp, vp, vp, u32, u32, vp, vp, ctypes.POINTER(StreamInfo),
                                                ctypes.POINTER(MultiSummary)]
        L.dvda_mlp_hip_set_conceal.argtypes = [vp, ctypes.c_int]
        L.dvda_mlp_hip_set_presentation.argtypes = [vp, u32]
        L.dvda_mlp_hip_segment_info.argtypes = [vp, u32, ctypes.POINTER(SegmentInfo), vp]
        L.dvda_mlp_hip_present_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64),
                                                ctypes.POINTER(u64)]
        L.dvda_mlp_hip_present_read.argtypes = [vp, vp, vp, u32, ctypes.POINTER(u64), vp, u64, u64, vp]
        L.dvda_mlp_hip_set_initial_fir.argtypes = [vp, vp]
        L.dvda_mlp_hip_segment_fir.argtypes = [vp, u32, vp, vp]
        L.dvda_mlp_hip_conceal_spans.argtypes = [vp, u32, ctypes.POINTER(ConcealSpan), u32, ctypes.POINTER(u32), vp]
        L.dvda_mlp_hip_conceal_edges.argtypes = [vp, u32, ctypes.POINTER(ConcealEdges), vp]
        L.dvda_pcm_hip_crc32_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_crc32_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_crc32.argtypes = [vp, u32, ctypes.c_uint, vp, u32, u64, vp, vp, vp, ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_crc32.argtypes = [vp, vp, vp, vp, ctypes.c_uint, vp, vp, u32, vp]
        L.dvda_pcm_hip_crc32_combine.restype = u32
        L.dvda_pcm_hip_crc32_combine.argtypes = [u32, u32, u64]
        L.dvda_pcm_hip_levels_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_levels_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_levels.argtypes = [vp, u32, ctypes.c_uint, vp, u32, u64, vp, vp, ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_levels.argtypes = [vp, vp, vp, vp, ctypes.c_uint, ctypes.POINTER(Levels), u32, vp]
        L.dvda_pcm_hip_levels_combine.restype = None
        L.dvda_pcm_hip_levels_combine.argtypes = [ctypes.POINTER(Levels), ctypes.POINTER(Levels), ctypes.POINTER(Levels)]
        L.dvda_pcm_hip_compare_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_compare_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_compare.argtypes = [vp, u32, vp, vp, u32, vp, u32, ctypes.c_uint, u64, vp, vp, ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_compare.argtypes = [vp, vp, vp, vp, vp, u32, vp, ctypes.c_uint, ctypes.POINTER(Diff), u32, vp]
        L.dvda_pcm_hip_diff_combine.argtypes = [ctypes.POINTER(Diff), ctypes.POINTER(Diff), ctypes.POINTER(Diff)]
        L.dvda_pcm_hip_energy_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_energy_workspace_words.argtypes = [u32, u64, u32]
        L.dvda_pcm_hip_energy.argtypes = [vp, u32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_energy.argtypes = [vp, vp, vp, vp, u32, ctypes.POINTER(EnergyBlock), u64, ctypes.POINTER(u64),
                                              u32, vp]
        L.dvda_pcm_hip_energy_append.argtypes = [ctypes.POINTER(EnergyBlock), ctypes.POINTER(u64), u64,
                                                 ctypes.POINTER(EnergyBlock), u64, u32]
        L.dvda_pcm_hip_energy_total.restype = None
        L.dvda_pcm_hip_energy_total.argtypes = [ctypes.POINTER(EnergyBlock), u64, ctypes.POINTER(EnergyBlock)]
        L.dvda_pcm_hip_requantize_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_requantize_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_requantize.argtypes = [vp, u32, vp, vp, u32, vp, vp, u32, ctypes.POINTER(Requant), u64, vp, vp,
                                              ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_requantize.argtypes = [vp, vp, vp, vp, ctypes.POINTER(Requant), ctypes.POINTER(u64),
                                                  ctypes.POINTER(RequantReport), u32, vp]
        L.dvda_pcm_hip_requant_value.restype = ctypes.c_int32
        L.dvda_pcm_hip_requant_value.argtypes = [ctypes.c_int32, u64, u32, ctypes.POINTER(Requant),
                                                 ctypes.POINTER(ctypes.c_int)]
        L.dvda_pcm_hip_decimate_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_decimate_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_decimate.argtypes = [vp, u32, vp, vp, u32, vp, vp, u32, u32, ctypes.c_uint, u64, vp, vp,
                                            ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_decimate.argtypes = [vp, vp, vp, vp, u32, ctypes.c_uint, vp, u32, ctypes.POINTER(u64),
                                                ctypes.POINTER(u64), ctypes.POINTER(DecimReport), u32, vp]
        L.dvda_pcm_hip_decim_taps.restype = ctypes.POINTER(ctypes.c_int32)
        L.dvda_pcm_hip_decim_taps.argtypes = [u32, ctypes.POINTER(u32)]
        L.dvda_pcm_hip_decim_out_frames.restype = u64
        L.dvda_pcm_hip_decim_out_frames.argtypes = [u64, u64, u32]
        L.dvda_pcm_hip_decim_value.restype = ctypes.c_int32
        L.dvda_pcm_hip_decim_value.argtypes = [vp, u32, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
        L.dvda_pcm_hip_resample_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_resample_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_resample.argtypes = [vp, u32, vp, vp, u32, vp, vp, u32, ctypes.c_uint, u64, vp, vp, ctypes.c_size_t,
                                            vp]
        L.dvda_mlp_hip_pcm_resample.argtypes = [vp, vp, vp, vp, ctypes.c_uint, vp, u32, ctypes.POINTER(u64),
                                                ctypes.POINTER(u64), vp, u32, vp]
        L.dvda_pcm_hip_resample_taps.restype = ctypes.POINTER(ctypes.c_int32)
        L.dvda_pcm_hip_resample_taps.argtypes = [ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.dvda_pcm_hip_resample_out_frames.restype = u64
        L.dvda_pcm_hip_resample_out_frames.argtypes = [u64, u64]
        L.dvda_pcm_hip_resample_value.restype = ctypes.c_int32
        L.dvda_pcm_hip_resample_value.argtypes = [vp, u32, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
        L.dvda_pcm_hip_mix_workspace_words.restype = ctypes.c_size_t
        L.dvda_pcm_hip_mix_workspace_words.argtypes = [u32, u64]
        L.dvda_pcm_hip_mix.argtypes = [vp, u32, vp, vp, u32, vp, vp, u32, ctypes.c_uint, u64, vp, vp, ctypes.c_size_t, vp]
        L.dvda_mlp_hip_pcm_mix.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(PcmMix), ctypes.c_uint,
                                           ctypes.POINTER(PcmMixReport), u32, vp]
        L.dvda_pcm_hip_speaker_mask.restype = ctypes.c_uint
        L.dvda_pcm_hip_speaker_mask.argtypes = [ctypes.c_uint]
        L.dvda_pcm_hip_mix_matrix.argtypes = [ctypes.c_uint, u32, u32, ctypes.POINTER(PcmMix)]
        L.dvda_pcm_hip_mix_valid.argtypes = [ctypes.POINTER(PcmMix)]
        L.dvda_pcm_hip_mix_value.restype = ctypes.c_int32
        L.dvda_pcm_hip_mix_value.argtypes = [vp, ctypes.POINTER(PcmMix), u32, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        names = {-1: "ENODEV", -2: "ENOMEM", -3: "EINVAL", -4: "ECAPACITY", -5: "ESTATE"}
        raise HipError("%s failed: %s (%d)" % (what, names.get(rc, "?"), rc))


PCM_PLANAR, PCM_INTERLEAVED, PCM_WAV24, PCM_WAV16 = 0, 1, 2, 3      # DVDA_PCM_* of include/dvda_mlp_hip.h
PRESENT_FULL, PRESENT_SUBSTREAM0 = 0, 1     # DVDA_PRESENT_*: the full decode / substream 0 alone, the 2-channel presentation
CHAIN_FORM = 0      # tests: 1 / 2 force the fused / two-pass form of the chain passes on every Context made afterwards


class Context:
    """One decode context = one GPU's index workspace (dvda_mlp_hip_create)."""

    def __init__(self, device=0, max_streams=1, max_segments=1024, lanes_per_segment=0, layout=PCM_PLANAR):
        self._h = ctypes.c_void_p()
        _check(lib().dvda_mlp_hip_create(ctypes.byref(self._h), device, max_streams, max_segments),
               "dvda_mlp_hip_create")
        self.set_lanes_per_segment(lanes_per_segment)
        self.set_pcm_layout(layout)
        if CHAIN_FORM:
            self.set_chain_form(CHAIN_FORM)
        self.device = device
        self.n_streams = 0
        self._batch = None

    def close(self):
        if self._h:
            lib().dvda_mlp_hip_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._batch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lanes_per_segment(self, lanes):
        _check(lib().dvda_mlp_hip_set_lanes_per_segment(self._h, lanes), "set_lanes")

    def set_pcm_layout(self, layout):
        _check(lib().dvda_mlp_hip_set_pcm_layout(self._h, layout), "set_pcm_layout")

    def set_chain_form(self, form):
        _check(lib().dvda_mlp_hip_set_chain_form(self._h, form), "set_chain_form")

    def set_presentation(self, presentation):
        """dvda_mlp_hip_set_presentation: PRESENT_FULL (default) or PRESENT_SUBSTREAM0 -- two-substream streams decode
        to the k-channel presentation substream 0 carries; asks for a new index()"""
        _check(lib().dvda_mlp_hip_set_presentation(self._h, presentation), "dvda_mlp_hip_set_presentation")

    def set_conceal(self, on):
        _check(lib().dvda_mlp_hip_set_conceal(self._h, int(on)), "dvda_mlp_hip_set_conceal")

    def set_initial_fir(self, d_fir_ptr):
        """device pointer to int32 [n_streams][2][48], the FIR history the streams start with, or None: fresh decoders"""
        _check(lib().dvda_mlp_hip_set_initial_fir(self._h, d_fir_ptr), "dvda_mlp_hip_set_initial_fir")

    def conceal_spans(self, i, stream=0):
        """spans of stream i from the last decode in conceal mode -> list of ConcealSpan.as_tuple()"""
        n = ctypes.c_uint32()
        _check(lib().dvda_mlp_hip_conceal_spans(self._h, i, None, 0, ctypes.byref(n), stream), "conceal_spans")
        arr = (ConcealSpan * max(int(n.value), 1))()
        _check(lib().dvda_mlp_hip_conceal_spans(self._h, i, arr, int(n.value), ctypes.byref(n), stream), "conceal_spans")
        return [arr[k].as_tuple() for k in range(int(n.value))]

    def conceal_edges(self, i, stream=0):
        """edges of stream i after the last decode in conceal mode -> ConcealEdges.as_dict(); HipError (ESTATE) when the
        last decode was not in conceal mode"""
        e = ConcealEdges()
        _check(lib().dvda_mlp_hip_conceal_edges(self._h, i, ctypes.byref(e), stream), "conceal_edges")
        return e.as_dict()

    def present_time(self):
        """-> (device ms of the strip kernels of the last index, source bytes, presentation bytes)"""
        ms, a, b = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().dvda_mlp_hip_present_time(self._h, ctypes.byref(ms), ctypes.byref(a), ctypes.byref(b)),
               "dvda_mlp_hip_present_time")
        return float(ms.value), int(a.value), int(b.value)

    def present_read(self, first=0, count=None, stream=0):
        """dvda_mlp_hip_present_read (diagnostic): the presentation buffer of the last index under PRESENT_SUBSTREAM0 ->
        (offsets, lengths: uint64 arrays per stream; readable: bytes of the buffer the call hands out; bytes
        [first, first + count) of it as a uint8 array, count=None: up to `readable`).  Blocks on `stream`; HipError
        (ESTATE) unless the context is indexed under the mode."""
        n = self.n_streams
        offs, lens = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        readable = ctypes.c_uint64()
        fn = lib().dvda_mlp_hip_present_read
        _check(fn(self._h, offs.ctypes.data, lens.ctypes.data, n, ctypes.byref(readable), None, 0, 0, stream),
               "dvda_mlp_hip_present_read")
        if count is None:
            count = int(readable.value) - first
        data = np.zeros(max(count, 0), np.uint8)
        _check(fn(self._h, None, None, 0, None, data.ctypes.data, first, count, stream), "dvda_mlp_hip_present_read")
        return offs, lens, int(readable.value), data

    def index(self, d_bytes_ptr, total_bytes, d_off_ptr, d_len_ptr, n_streams, stream=0):
        self.n_streams = n_streams
        _check(lib().dvda_mlp_hip_index(self._h, d_bytes_ptr, total_bytes, d_off_ptr, d_len_ptr,
                                        n_streams, stream), "dvda_mlp_hip_index")

    def index_batch(self, batch, stream=0):
        """index() of a Batch.  The library keeps the pointers, not the bytes, and the decode reads through them: the
        context holds on to `batch` until the next index_batch() or close(), so it cannot be freed under a live index"""
        self._batch = batch
        self.index(batch.d_bytes.data_ptr(), batch.total, batch.d_off.data_ptr(), batch.d_len.data_ptr(), batch.n, stream)

    def decode(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, stream=0):
        _check(lib().dvda_mlp_hip_decode(self._h, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, stream),
               "dvda_mlp_hip_decode")

    def decode_async(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, stream=0):
        """dvda_mlp_hip_decode_async: every pass enqueued, no host wait, no allocation (see reserve)."""
        _check(lib().dvda_mlp_hip_decode_async(self._h, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, stream),
               "dvda_mlp_hip_decode_async")

    def reserve(self, chain_pcm_frames=0, chain_segments=0, seq_streams=0):
        _check(lib().dvda_mlp_hip_reserve(self._h, chain_pcm_frames, chain_segments, seq_streams), "dvda_mlp_hip_reserve")

    def stream_info(self, n=None, stream=0):
        n = self.n_streams if n is None else n
        arr = (StreamInfo * n)()
        _check(lib().dvda_mlp_hip_stream_info(self._h, arr, n, stream), "dvda_mlp_hip_stream_info")
        return arr

    def segment_count(self, stream=0):
        v = ctypes.c_uint32()
        _check(lib().dvda_mlp_hip_segment_count(self._h, ctypes.byref(v), stream), "segment_count")
        return int(v.value)

    def index_graph_state(self):
        """dvda_mlp_hip_index_graph_state: 1 the last index was launched directly and its key noted, 2 it went out as a
        hipGraph (captured or replayed), -1 the graph is off for this context, 0 nothing noted yet"""
        v = ctypes.c_int()
        _check(lib().dvda_mlp_hip_index_graph_state(self._h, ctypes.byref(v)), "index_graph_state")
        return int(v.value)

    def segment_info(self, segment, stream=0):
        info = SegmentInfo()
        _check(lib().dvda_mlp_hip_segment_info(self._h, segment, ctypes.byref(info), stream), "segment_info")
        return info

    def segment_fir(self, segment, stream=0):
        """FIR history [2][48] at the end of `segment` (dvda_mlp_hip_segment_fir)"""
        fir = np.zeros((2, 48), np.int32)
        _check(lib().dvda_mlp_hip_segment_fir(self._h, segment, fir.ctypes.data, stream), "segment_fir")
        return fir

    def pcm_crc32(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, bits, n=None, stream=0):
        """dvda_mlp_hip_pcm_crc32: zlib CRC-32 of every stream's WAV payload at `bits`, computed on the device from the
        PCM the last decode wrote -> list of (crc, payload bytes); blocks"""
        n = self.n_streams if n is None else n
        crc = np.zeros(n, np.uint32)
        nbytes = np.zeros(n, np.uint64)
        _check(lib().dvda_mlp_hip_pcm_crc32(self._h, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, bits, crc.ctypes.data,
                                            nbytes.ctypes.data, n, stream), "dvda_mlp_hip_pcm_crc32")
        return [(int(c), int(b)) for c, b in zip(crc, nbytes)]

    def _records(self, name, cls, n, stream, *args):
        """what the pcm_* calls have in common: lib().<name>(context, *args, room for n records of cls, n, stream),
        checked -> list of cls.as_dict()"""
        arr = (cls * max(n, 1))()
        _check(getattr(lib(), name)(self._h, *args, arr, n, stream), name)
        return [arr[i].as_dict() for i in range(n)]

    def pcm_levels(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, bits, n=None, stream=0):
        """dvda_mlp_hip_pcm_levels: the level report of every stream at nominal depth `bits` (16, 20 or 24), computed on
        the device from the int32 PCM the last decode wrote -> list of Levels.as_dict(); blocks.  HipError (EINVAL) when
        the context's layout is a WAV one."""
        n = self.n_streams if n is None else n
        return self._records("dvda_mlp_hip_pcm_levels", Levels, n, stream, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, bits)

    def pcm_energy(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, block_frames, n=None, stream=0, cap_blocks=None):
        """dvda_mlp_hip_pcm_energy: per block of block_frames frames and channel the exact sum of squares and the peak
        of every stream, computed on the device from the int32 PCM the last decode wrote -> one list of
        EnergyBlock.as_dict() per stream; blocks.  cap_blocks: room for that many blocks in all (HipError ECAPACITY
        when it is too small); default: the call asks first how many there are.  HipError (EINVAL) when the context's
        layout is a WAV one."""
        n = self.n_streams if n is None else n
        first = (ctypes.c_uint64 * (n + 1))()
        fn = lib().dvda_mlp_hip_pcm_energy
        if cap_blocks is None:
            rc = fn(self._h, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, block_frames, None, 0, first, n, stream)
            if rc not in (0, -4):
                _check(rc, "dvda_mlp_hip_pcm_energy")
            cap_blocks = int(first[n])
        arr = (EnergyBlock * max(cap_blocks, 1))()
        _check(fn(self._h, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, block_frames, arr, cap_blocks, first, n, stream),
               "dvda_mlp_hip_pcm_energy")
        return [[arr[j].as_dict() for j in range(int(first[i]), int(first[i + 1]))] for i in range(n)]

    def pcm_compare(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, d_other, other_layout, other_desc, bits=0, n=None,
                    stream=None):
        """dvda_mlp_hip_pcm_compare: the first n streams of the last decode (side A, where the decode wrote them) against
        the streams of d_other, an int32 device tensor in other_layout with other_desc a list of (off, stride, frames,
        channels) (side B) -> list of Diff.as_dict(); blocks.  bits: 0 -- the int32 values as they are -- or 16 / 20 / 24:
        the values as they would be written.  stream: default torch's current one on this context's device.  HipError
        (EINVAL) when the context's layout is a WAV one."""
        import torch
        n = self.n_streams if n is None else n
        if len(other_desc) < n:
            raise HipError("pcm_compare: %d descriptors for %d streams" % (len(other_desc), n))
        if stream is None:
            stream = torch.cuda.current_stream(d_other.device).cuda_stream
        d_desc = _to_device(_desc_records(other_desc[:n]), d_other.device)
        return self._records("dvda_mlp_hip_pcm_compare", Diff, n, stream, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr,
                             d_other.data_ptr(), other_layout, d_desc.data_ptr(), bits)

    def pcm_requantize(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, bits_in, bits_out, mode=RQ_TPDF, seed=0,
                       frame0=None, n=None, stream=0):
        """dvda_mlp_hip_pcm_requantize: the int32 PCM the last decode wrote, reduced IN PLACE from bits_in to bits_out
        (truncated, rounded or dithered; clamped) -> list of RequantReport.as_dict(); blocks.  frame0: per stream the
        absolute frame it starts at (None: 0).  HipError (EINVAL) when the context's layout is a WAV one."""
        n = self.n_streams if n is None else n
        f0 = None if frame0 is None else (ctypes.c_uint64 * max(n, 1))(*[int(f) for f in frame0][:n])
        par = Requant(bits_in, bits_out, mode, 0, seed)
        return self._records("dvda_mlp_hip_pcm_requantize", RequantReport, n, stream, d_pcm_ptr, d_out_off_ptr,
                             d_out_stride_ptr, ctypes.byref(par), f0)

    def pcm_decimate(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, ratio, bits, d_dst_ptr, layout_dst, dst_off,
                     dst_stride, n=None, stream=0):
        """dvda_mlp_hip_pcm_decimate: the int32 PCM the last decode wrote, whole tracks, decimated by `ratio` (2 or 4) and
        clamped to `bits` into the device buffer at d_dst_ptr in layout_dst (PCM_PLANAR or PCM_INTERLEAVED): stream i to
        the int32 word dst_off[i], planar stride dst_stride[i] (host lists) -> list of DecimReport.as_dict(); blocks.
        HipError (EINVAL) when the context's layout is a WAV one."""
        n = self.n_streams if n is None else n
        off = (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in dst_off][:n])
        stride = (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in dst_stride][:n])
        return self._records("dvda_mlp_hip_pcm_decimate", DecimReport, n, stream, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr,
                             ratio, bits, d_dst_ptr, layout_dst, off, stride)

    def pcm_resample(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, bits, d_dst_ptr, layout_dst, dst_off, dst_stride,
                     n=None, stream=0):
        """dvda_mlp_hip_pcm_resample: the int32 PCM the last decode wrote, whole tracks taken as 48 kHz, resampled to
        44.1 kHz and clamped to `bits` into the device buffer at d_dst_ptr in layout_dst (PCM_PLANAR or PCM_INTERLEAVED):
        stream i to the int32 word dst_off[i], planar stride dst_stride[i] (host lists) -> list of
        DecimReport.as_dict(); blocks.  HipError (EINVAL) when the context's layout is a WAV one."""
        n = self.n_streams if n is None else n
        off = (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in dst_off][:n])
        stride = (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in dst_stride][:n])
        return self._records("dvda_mlp_hip_pcm_resample", DecimReport, n, stream, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr,
                             bits, d_dst_ptr, layout_dst, off, stride)

    def pcm_mix(self, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr, d_dst_ptr, d_mix_off_ptr, d_mix_stride_ptr, matrices, bits,
                n=None, stream=0):
        """dvda_mlp_hip_pcm_mix: the int32 PCM the last decode wrote, stream i mixed through matrices[i] (a PcmMix or its
        dict) and clamped to `bits` into the device buffer at d_dst_ptr, in the context's layout: to the int32 word
        d_mix_off[i] with the planar stride d_mix_stride[i] (device arrays of uint64, as d_out_off / d_out_stride are) ->
        list of PcmMixReport.as_dict(); blocks.  HipError (EINVAL) when the context's layout is a WAV one."""
        n = self.n_streams if n is None else n
        if len(matrices) < n:
            raise HipError("pcm_mix: %d matrices for %d streams" % (len(matrices), n))
        mats = (PcmMix * max(n, 1))(*[_mix_record(m) for m in matrices[:n]])
        return self._records("dvda_mlp_hip_pcm_mix", PcmMixReport, n, stream, d_pcm_ptr, d_out_off_ptr, d_out_stride_ptr,
                             d_dst_ptr, d_mix_off_ptr, d_mix_stride_ptr, mats, bits)

    def decode_time(self):
        """mean device ms of a whole decode call (all passes); call before kernel_time(), which resets the ring"""
        ms = ctypes.c_double()
        n = ctypes.c_uint32()
        _check(lib().dvda_mlp_hip_decode_time(self._h, ctypes.byref(ms), ctypes.byref(n)), "decode_time")
        return float(ms.value), int(n.value)

    def kernel_time(self):
        ms = ctypes.c_double()
        n = ctypes.c_uint32()
        _check(lib().dvda_mlp_hip_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(n)), "kernel_time")
        return float(ms.value), int(n.value)


def crc32_combine(crc_a, crc_b, len_b):
    """dvda_pcm_hip_crc32_combine: crc(A || B) from crc(A), crc(B) and len(B); host arithmetic, needs no GPU"""
    return int(lib().dvda_pcm_hip_crc32_combine(crc_a, crc_b, len_b))


def _desc_records(desc):
    """a list of (off, stride, frames, channels) -> the dvda_pcm_crc_desc records (one at least, so that it has an address)"""
    rec = np.zeros(max(len(desc), 1), np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"),
                                                 ("reserved", "<u4")]))
    for i, (off, stride, frames, channels) in enumerate(desc):
        rec[i] = (off, stride, frames, channels, 0)
    return rec


def _to_device(rec, dev):
    """a numpy array of records (_desc_records, _piece_records) -> its bytes on `dev` (the host waits for the copy)"""
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)


def _result_tensor(cls, n, dev):
    """room on `dev` for n records of cls (one at least, so that it has an address), zeroed: uint8 [max(n, 1), sizeof(cls)]"""
    import torch
    return torch.zeros((max(n, 1), ctypes.sizeof(cls)), dtype=torch.uint8, device=dev)


def _record_list(cls, d_records):
    """a uint8 device tensor [n, sizeof(cls)] -> list of cls.as_dict() on the host (waits)"""
    raw = np.ascontiguousarray(d_records.cpu().numpy())
    return [cls.from_buffer_copy(raw[i].tobytes()).as_dict() for i in range(raw.shape[0])]


def _report_args(d_pcm, desc, what, max_total, work, workspace_words):
    """What pcm_crc32 and pcm_levels hand their C entry point besides the results: the dvda_pcm_crc_desc records of `desc`
    on d_pcm's device (the host waits for that copy), the workspace (`work`, or one allocated here from
    workspace_words(n, max_total)) and torch's current stream.  -> (torch, n, d_desc, work, stream)"""
    import torch
    if not torch.cuda.is_available():
        raise HipError("no GPU visible to torch: %s is HIP-only" % what)
    dev = d_pcm.device
    n = len(desc)
    if work is None:
        work = torch.empty(int(workspace_words(n, max_total)), dtype=torch.int32, device=dev)
    return torch, n, _to_device(_desc_records(desc), dev), work, torch.cuda.current_stream(dev).cuda_stream


def pcm_crc32(d_pcm, layout, bits, desc, max_total_bytes=None, work=None):
    """dvda_pcm_hip_crc32 over torch tensors: d_pcm an int32 tensor on the device holding the streams in `layout`,
    desc a list of (off, stride, frames, channels) as dvda_pcm_crc_desc states them.  -> (crc, nbytes): device tensors
    (int32 bit patterns of the CRCs, int64 byte counts).  Only the kernels are asynchronous, on torch's current stream:
    this helper builds the descriptors on the host and copies them to the device (the host waits for that copy), and
    allocates them, the two results and -- when none is passed -- the workspace; a caller that must not wait or
    allocate keeps those on the device and calls dvda_pcm_hip_crc32 itself (tools/digest_bench.py).
    max_total_bytes: bound on the sum of the payload bytes (default: computed from desc); work: an int32 workspace
    tensor of at least pcm_crc32_workspace_words() elements (default: allocated here)."""
    if max_total_bytes is None:
        max_total_bytes = int(sum(int(f) * int(c) * (bits // 8) for _, _, f, c in desc))
    torch, n, d_desc, work, st = _report_args(d_pcm, desc, "the PCM digest", max_total_bytes, work,
                                              lib().dvda_pcm_hip_crc32_workspace_words)
    d_crc = torch.zeros(max(n, 1), dtype=torch.int32, device=d_pcm.device)
    d_nbytes = torch.zeros(max(n, 1), dtype=torch.int64, device=d_pcm.device)
    _check(lib().dvda_pcm_hip_crc32(d_pcm.data_ptr(), layout, bits, d_desc.data_ptr(), n, max_total_bytes,
                                    d_crc.data_ptr(), d_nbytes.data_ptr(), work.data_ptr(), work.numel(), st),
           "dvda_pcm_hip_crc32")
    return d_crc[:n], d_nbytes[:n]


def pcm_crc32_workspace_words(n, max_total_bytes):
    return int(lib().dvda_pcm_hip_crc32_workspace_words(n, max_total_bytes))


def levels_combine(a, b):
    """dvda_pcm_hip_levels_combine: the report of A || B from the reports of A and B (dicts as Levels.as_dict() gives
    them); host arithmetic, needs no GPU"""
    out = Levels()
    lib().dvda_pcm_hip_levels_combine(ctypes.byref(Levels.from_dict(a)), ctypes.byref(Levels.from_dict(b)),
                                      ctypes.byref(out))
    return out.as_dict()


def pcm_levels(d_pcm, layout, bits, desc, max_total_frames=None, work=None):
    """dvda_pcm_hip_levels over torch tensors: d_pcm an int32 tensor on the device holding the streams in `layout`
    (PCM_PLANAR or PCM_INTERLEAVED), desc a list of (off, stride, frames, channels) as dvda_pcm_crc_desc states them.
    -> a uint8 device tensor [n, sizeof(Levels)] (levels_list brings it to the host).  Only the kernels are
    asynchronous, on torch's current stream: like pcm_crc32, this helper builds the descriptors on the host, copies them
    to the device and allocates them, the result and -- when none is passed -- the workspace.
    max_total_frames: bound on the sum of the frames (default: computed from desc); work: an int32 workspace tensor of at
    least pcm_levels_workspace_words() elements (default: allocated here)."""
    if max_total_frames is None:
        max_total_frames = int(sum(int(f) for _, _, f, c in desc if 1 <= int(c) <= 8))
    torch, n, d_desc, work, st = _report_args(d_pcm, desc, "the level report", max_total_frames, work,
                                              lib().dvda_pcm_hip_levels_workspace_words)
    d_out = _result_tensor(Levels, n, d_pcm.device)
    _check(lib().dvda_pcm_hip_levels(d_pcm.data_ptr(), layout, bits, d_desc.data_ptr(), n, max_total_frames,
                                     d_out.data_ptr(), work.data_ptr(), work.numel(), st), "dvda_pcm_hip_levels")
    return d_out[:n]


def pcm_levels_workspace_words(n, max_total_frames):
    return int(lib().dvda_pcm_hip_levels_workspace_words(n, max_total_frames))


def levels_list(d_levels):
    """pcm_levels' tensor -> list of Levels.as_dict() on the host (waits)"""
    return _record_list(Levels, d_levels)


def _compared(da, db):
    """frames a pair of (off, stride, frames, channels) compares, as the kernels judge the descriptors"""
    ok = da[3] == db[3] and 1 <= int(da[3]) <= 8 and max(int(da[2]), int(db[2])) <= 1 << 40
    return min(int(da[2]), int(db[2])) if ok else 0


def pcm_compare(d_a, layout_a, desc_a, d_b, layout_b, desc_b, bits=0, max_total_frames=None, work=None):
    """dvda_pcm_hip_compare over torch tensors: d_a / d_b int32 tensors on one device holding the streams of side A / B in
    layout_a / layout_b (PCM_PLANAR or PCM_INTERLEAVED, chosen per side), desc_a / desc_b lists of (off, stride, frames,
    channels) of the same length: stream i of A is compared with stream i of B.  bits: 0 -- the int32 values as they
    are -- or 16 / 20 / 24: as they would be written.  -> a uint8 device tensor [n, sizeof(Diff)] (diff_list brings it to
    the host).  Only the kernels are asynchronous, on torch's current stream: like pcm_levels, this helper builds the
    descriptors on the host, copies them to the device and allocates them, the result and -- when none is passed -- the
    workspace.  max_total_frames: bound on the sum of the frames compared (default: computed from both descriptor
    lists); work: an int32 workspace tensor of at least pcm_compare_workspace_words() elements."""
    if len(desc_a) != len(desc_b):
        raise HipError("pcm_compare: %d descriptors against %d" % (len(desc_a), len(desc_b)))
    if max_total_frames is None:
        max_total_frames = int(sum(_compared(a, b) for a, b in zip(desc_a, desc_b)))
    torch, n, d_desc_a, work, st = _report_args(d_a, desc_a, "the PCM compare", max_total_frames, work,
                                                lib().dvda_pcm_hip_compare_workspace_words)
    d_desc_b = _to_device(_desc_records(desc_b), d_a.device)
    d_out = _result_tensor(Diff, n, d_a.device)
    _check(lib().dvda_pcm_hip_compare(d_a.data_ptr(), layout_a, d_desc_a.data_ptr(), d_b.data_ptr(), layout_b,
                                      d_desc_b.data_ptr(), n, bits, max_total_frames, d_out.data_ptr(), work.data_ptr(),
                                      work.numel(), st), "dvda_pcm_hip_compare")
    return d_out[:n]


def pcm_compare_workspace_words(n, max_total_frames):
    return int(lib().dvda_pcm_hip_compare_workspace_words(n, max_total_frames))


def diff_list(d_diff):
    """pcm_compare's tensor -> list of Diff.as_dict() on the host (waits)"""
    return _record_list(Diff, d_diff)


def diff_combine(a, b):
    """dvda_pcm_hip_diff_combine: the diff of A1 || A2 against B1 || B2 from the diffs of the two pieces (dicts as
    Diff.as_dict() gives them); host arithmetic, needs no GPU.  HipError (EINVAL) when the pieces do not line up"""
    out = Diff()
    _check(lib().dvda_pcm_hip_diff_combine(ctypes.byref(Diff.from_dict(a)), ctypes.byref(Diff.from_dict(b)),
                                           ctypes.byref(out)), "dvda_pcm_hip_diff_combine")
    return out.as_dict()


def energy_nblocks(frames, block_frames, lead=None):
    """blocks of a stream of `frames` frames on the grid (block_frames, lead): the rule of include/dvda_mlp_hip.h"""
    lead = block_frames if lead is None else lead
    if frames <= 0 or not 1 <= lead <= block_frames:
        return 0
    return 1 + -(-max(frames - lead, 0) // block_frames)


def pcm_energy(d_pcm, layout, desc, block_frames, lead=None, max_total_frames=None, work=None, caps=None):
    """dvda_pcm_hip_energy over torch tensors: d_pcm an int32 tensor on the device holding the streams in `layout`
    (PCM_PLANAR or PCM_INTERLEAVED), desc a list of (off, stride, frames, channels) as dvda_pcm_crc_desc states them,
    block_frames the grid's block length and lead the first block's length per stream (None: block_frames for all).
    -> (d_blocks, first, d_nblocks): a uint8 device tensor [first[-1], sizeof(EnergyBlock)] in which stream i has room for
    the blocks first[i] .. first[i + 1], that list, and an int64 device tensor of the streams' block counts
    (energy_lists brings all of it to the host).  caps: room per stream (default: what each needs by energy_nblocks).
    Only the kernels are asynchronous, on torch's current stream: like pcm_levels, this helper builds the descriptors on
    the host, copies them to the device and allocates them, the results and -- when none is passed -- the workspace.
    max_total_frames: bound on the sum of the frames (default: computed from desc); work: an int32 workspace tensor of
    at least pcm_energy_workspace_words() elements."""
    taken = [1 <= int(c) <= 8 and int(f) <= 1 << 40 for _, _, f, c in desc]
    if max_total_frames is None:
        max_total_frames = int(sum(int(d[2]) for d, ok in zip(desc, taken) if ok))
    torch, n, d_desc, work, st = _report_args(d_pcm, desc, "the energy report", max_total_frames, work,
                                              lambda k, total: lib().dvda_pcm_hip_energy_workspace_words(k, total,
                                                                                                         block_frames))
    dev = d_pcm.device
    if caps is None:
        caps = [energy_nblocks(int(d[2]), block_frames, None if lead is None else int(lead[i])) if ok else 0
                for i, (d, ok) in enumerate(zip(desc, taken))]
    first = [0]
    for c in caps:
        first.append(first[-1] + int(c))
    arr = torch.tensor([first[:n] + [0], [int(c) for c in caps] + [0]], dtype=torch.int64).to(dev)
    d_lead = None if lead is None else torch.tensor([int(v) for v in lead] + [0], dtype=torch.int32).to(dev)
    d_blocks = _result_tensor(EnergyBlock, first[-1], dev)
    d_nblocks = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    _check(lib().dvda_pcm_hip_energy(d_pcm.data_ptr(), layout, d_desc.data_ptr(), n, block_frames,
                                     None if d_lead is None else d_lead.data_ptr(), max_total_frames, d_blocks.data_ptr(),
                                     arr[0].data_ptr(), arr[1].data_ptr(), d_nblocks.data_ptr(), work.data_ptr(),
                                     work.numel(), st), "dvda_pcm_hip_energy")
    return d_blocks[:first[-1]], first, d_nblocks[:n]


def pcm_energy_workspace_words(n, max_total_frames, block_frames):
    return int(lib().dvda_pcm_hip_energy_workspace_words(n, max_total_frames, block_frames))


def energy_lists(d_blocks, first, d_nblocks):
    """pcm_energy's results -> (one list of EnergyBlock.as_dict() per stream: the blocks that were written, the block
    counts as the device reports them) on the host (waits)"""
    raw = np.ascontiguousarray(d_blocks.cpu().numpy())
    counts = [int(v) for v in d_nblocks.cpu().numpy()]
    out = []
    for i, nb in enumerate(counts):
        room = first[i + 1] - first[i]
        out.append([EnergyBlock.from_buffer_copy(raw[first[i] + j].tobytes()).as_dict() for j in range(min(nb, room))])
    return out, counts


def _energy_array(blocks):
    arr = (EnergyBlock * max(len(blocks), 1))()
    for j, b in enumerate(blocks):
        arr[j] = EnergyBlock.from_dict(b)
    return arr


def energy_append(track, piece, block_frames, cap=None):
    """dvda_pcm_hip_energy_append: the blocks of a track (a list of EnergyBlock.as_dict()) with a piece's blocks joined
    to them -> the new list; host arithmetic, needs no GPU.  cap: the room the track's array has (default: enough).
    HipError EINVAL when the piece is not on the track's grid, ECAPACITY when cap is too small."""
    cap = len(track) + len(piece) if cap is None else cap
    arr = (EnergyBlock * max(cap, len(track), 1))()
    for j, b in enumerate(track):
        arr[j] = EnergyBlock.from_dict(b)
    n = ctypes.c_uint64(len(track))
    _check(lib().dvda_pcm_hip_energy_append(arr, ctypes.byref(n), cap, _energy_array(piece), len(piece), block_frames),
           "dvda_pcm_hip_energy_append")
    return [arr[j].as_dict() for j in range(int(n.value))]


def energy_total(blocks):
    """dvda_pcm_hip_energy_total: the blocks folded into one record (frames saturates at 2^32 - 1); needs no GPU"""
    out = EnergyBlock()
    lib().dvda_pcm_hip_energy_total(_energy_array(blocks), len(blocks), ctypes.byref(out))
    return out.as_dict()


def energy_sums(blocks):
    """per block the eight sums of squares as Python ints (sq_hi << 64 | sq_lo)"""
    return [[(int(h) << 64) | int(l) for l, h in zip(b["sq_lo"], b["sq_hi"])] for b in blocks]


def pcm_requantize(d_in, layout_in, desc_in, bits_in, bits_out, mode=RQ_TPDF, seed=0, frame0=None, out=None,
                   layout_out=None, desc_out=None, max_total_frames=None, work=None):
    """dvda_pcm_hip_requantize over torch tensors: d_in an int32 tensor on the device holding the streams in layout_in
    (PCM_PLANAR or PCM_INTERLEAVED), desc_in a list of (off, stride, frames, channels); every value reduced from bits_in to
    bits_out bits (mode: RQ_TRUNCATE, RQ_ROUND, RQ_TPDF with `seed`) and clamped.  frame0: per stream the absolute frame
    it starts at (None: 0).  out / layout_out / desc_out: where the result goes -- default: the input's layout and
    descriptors in a fresh tensor of the same placement (a copy of d_in for an int32 layout, zeros for PCM_WAV16 /
    PCM_WAV24); out=d_in with the same layout and descriptors works in place.  -> (d_out, d_report): the output tensor
    and a uint8 device tensor [n, sizeof(RequantReport)] (requant_list brings it to the host).  Only the kernels are
    asynchronous, on torch's current stream: like pcm_levels, this helper builds the descriptors on the host, copies
    them to the device and allocates them, the results and -- when none is passed -- the workspace."""
    layout_out = layout_in if layout_out is None else layout_out
    desc_out = desc_in if desc_out is None else desc_out
    if len(desc_out) != len(desc_in):
        raise HipError("pcm_requantize: %d output descriptors for %d streams" % (len(desc_out), len(desc_in)))
    if max_total_frames is None:
        max_total_frames = int(sum(int(f) for _, _, f, c in desc_in if 1 <= int(c) <= 8 and int(f) <= 1 << 40))
    torch, n, d_desc_in, work, st = _report_args(d_in, desc_in, "the word-length reduction", max_total_frames, work,
                                                 lib().dvda_pcm_hip_requantize_workspace_words)
    dev = d_in.device
    if out is None:
        out = d_in.clone() if layout_out in (PCM_PLANAR, PCM_INTERLEAVED) else torch.zeros_like(d_in)
    d_desc_out = _to_device(_desc_records(desc_out), dev)
    d_f0 = None if frame0 is None else torch.from_numpy(
        np.array([int(f) for f in frame0] + [0], np.uint64).view(np.int64)).to(dev)
    d_rep = _result_tensor(RequantReport, n, dev)
    par = Requant(bits_in, bits_out, mode, 0, seed)
    _check(lib().dvda_pcm_hip_requantize(d_in.data_ptr(), layout_in, d_desc_in.data_ptr(), out.data_ptr(), layout_out,
                                         d_desc_out.data_ptr(), None if d_f0 is None else d_f0.data_ptr(), n,
                                         ctypes.byref(par), max_total_frames, d_rep.data_ptr(), work.data_ptr(),
                                         work.numel(), st), "dvda_pcm_hip_requantize")
    return out, d_rep[:n]


def pcm_requantize_workspace_words(n, max_total_frames):
    return int(lib().dvda_pcm_hip_requantize_workspace_words(n, max_total_frames))


def requant_list(d_report):
    """pcm_requantize's report tensor -> list of RequantReport.as_dict() on the host (waits)"""
    return _record_list(RequantReport, d_report)


def _value_call(name, invalid, *args):
    """what the *_value wrappers have in common: lib().<name>(*args, &clipped) -> (value, clipped); HipError naming
    `invalid` where the call says its parameters are (clipped < 0)"""
    cl = ctypes.c_int(0)
    y = getattr(lib(), name)(*args, ctypes.byref(cl))
    if cl.value < 0:
        raise HipError("%s: invalid parameters %s" % (name, invalid))
    return int(y), int(cl.value)


def requant_value(v, frame, channel, bits_in, bits_out, mode=RQ_TPDF, seed=0):
    """dvda_pcm_hip_requant_value: the word-length reduction of one value at absolute frame `frame` of channel `channel`
    -> (value, 1 when the clamp changed it else 0); host arithmetic, needs no GPU.  HipError for invalid parameters"""
    par = Requant(bits_in, bits_out, mode, 0, seed)
    return _value_call("dvda_pcm_hip_requant_value", "%r" % (par.as_dict(),), int(v), frame, channel, ctypes.byref(par))


def decim_taps(ratio):
    """dvda_pcm_hip_decim_taps: the committed tap table of `ratio` as an int32 array (a copy); needs no GPU.  HipError
    for a ratio other than 2 or 4"""
    n = ctypes.c_uint32(0)
    p = lib().dvda_pcm_hip_decim_taps(ratio, ctypes.byref(n))
    if not p or not n.value:
        raise HipError("dvda_pcm_hip_decim_taps: no table for ratio %r" % (ratio,))
    return np.ctypeslib.as_array(p, (int(n.value),)).astype(np.int32)


def decim_out_frames(frame0, own, ratio):
    """dvda_pcm_hip_decim_out_frames: output frames of the absolute frames [frame0, frame0 + own); needs no GPU"""
    return int(lib().dvda_pcm_hip_decim_out_frames(frame0, own, ratio))


def decim_value(window, ratio, bits):
    """dvda_pcm_hip_decim_value: one output value from its window of 2 H + 1 input values -> (value, 1 when the clamp
    changed it else 0); host arithmetic, needs no GPU.  HipError for an invalid ratio or depth or a window of another
    length"""
    w = np.ascontiguousarray(window, np.int32)
    if ratio not in (2, 4) or w.shape != (96 * ratio - 1,):
        raise HipError("dvda_pcm_hip_decim_value: a window of %s values for ratio %r" % (w.shape, ratio))
    return _value_call("dvda_pcm_hip_decim_value", "(ratio %r, bits %r)" % (ratio, bits), w.ctypes.data, ratio, bits)


def _piece_records(pieces):
    """a list of (frame0, before, after) -> the dvda_pcm_decim_piece records (one at least)"""
    rec = np.zeros(max(len(pieces), 1), np.dtype([("frame0", "<u8"), ("before", "<u4"), ("after", "<u4")]))
    for i, (frame0, before, after) in enumerate(pieces):
        rec[i] = (frame0, before, after)
    return rec


def _end_to_end(desc_in, frames_and_channels):
    """the output descriptors a writer makes when none are passed: stream i of `frames` frames and `ch` channels gives
    frames_and_channels(i, frames, ch, ok) = (its output frames, its output channels), ok saying whether a pass takes the
    input descriptor at all (where not, it asks the library nothing and gives no frames); the regions end to end with the
    stride = the frames, which serves either int32 layout -> (desc_out, words)"""
    out, pos = [], 0
    for i, (_, _, frames, ch) in enumerate(desc_in):
        f, c = frames_and_channels(i, int(frames), int(ch), 1 <= int(ch) <= 8 and int(frames) <= 1 << 40)
        out.append((pos, f, f, c))
        pos += f * c
    return out, max(pos, 1)


def _writer_call(name, cname, what, cls, d_in, layout_in, desc_in, extra, params, out, layout_out, desc_out, default_desc,
                 bound_in, max_total, work):
    """What pcm_decimate, pcm_resample and pcm_mix (`name`) do around their entry point `cname` and its
    <cname>_workspace_words: the defaults of layout_out and desc_out (default_desc() -> (desc_out, words)), the bound (the
    frames the pass takes of desc_in where bound_in, else of desc_out), _report_args, the zeroed output, the device copies
    of desc_out and of extra() (the pieces' or matrices' records; None: none), room for n records of cls, and the call:
    (d_in, layout_in, desc_in, out, layout_out, desc_out, extra, n, *params, bound, report, work, words, stream).
    -> (d_out, desc_out, d_report)"""
    layout_out = layout_in if layout_out is None else layout_out
    words = None
    if desc_out is None:
        desc_out, words = default_desc()
    if len(desc_out) != len(desc_in):
        raise HipError("%s: %d output descriptors for %d streams" % (name, len(desc_out), len(desc_in)))
    if max_total is None:
        bound = desc_in if bound_in else desc_out
        max_total = int(sum(int(f) for _, _, f, c in bound if 1 <= int(c) <= 8 and int(f) <= 1 << 40))
    torch, n, d_desc_in, work, st = _report_args(d_in, desc_in, what, max_total, work, getattr(lib(), cname + "_workspace_words"))
    dev = d_in.device
    if out is None:
        if words is None:
            words = max([int(o) + int(r) * int(c) for o, r, f, c in desc_out] + [1])
        out = torch.zeros(words, dtype=torch.int32, device=dev)
    d_desc_out = _to_device(_desc_records(desc_out), dev)
    d_extra = None if extra is None else _to_device(extra(), dev)
    d_rep = _result_tensor(cls, n, dev)
    _check(getattr(lib(), cname)(d_in.data_ptr(), layout_in, d_desc_in.data_ptr(), out.data_ptr(), layout_out,
                                 d_desc_out.data_ptr(), None if d_extra is None else d_extra.data_ptr(), n, *params, max_total,
                                 d_rep.data_ptr(), work.data_ptr(), work.numel(), st), cname)
    return out, desc_out, d_rep[:n]


def decim_desc_out(desc_in, ratio, pieces=None):
    """the output descriptors pcm_decimate makes when none are passed: per stream its output frames (0 for a stream the
    pass does not take), the input's channels, the regions end to end with the stride = the frames, which serves either
    int32 layout -> (desc_out, words)"""
    def shape(i, frames, ch, ok):
        frame0, before, after = pieces[i] if pieces is not None else (0, 0, 0)
        return (decim_out_frames(frame0, frames - before - after, ratio) if ok and before + after <= frames else 0), ch
    return _end_to_end(desc_in, shape)


def pcm_decimate(d_in, layout_in, desc_in, ratio, bits, pieces=None, out=None, layout_out=None, desc_out=None,
                 max_total_out_frames=None, work=None):
    """dvda_pcm_hip_decimate over torch tensors: d_in an int32 tensor on the device holding the streams in layout_in
    (PCM_PLANAR or PCM_INTERLEAVED), desc_in a list of (off, stride, frames, channels); every stream decimated by `ratio`
    (2 or 4), the values clamped to `bits`.  pieces: per stream (frame0, before, after) as dvda_pcm_decim_piece states
    them (None: whole tracks).  out / layout_out / desc_out: where the result goes -- default: the input's layout, the
    regions end to end in a fresh zeroed tensor (decim_desc_out).  -> (d_out, desc_out, d_report): the output tensor, its
    descriptors and a uint8 device tensor [n, sizeof(DecimReport)] (decim_list brings it to the host).  Only the kernels
    are asynchronous, on torch's current stream: like pcm_levels, this helper builds the descriptors on the host, copies
    them to the device and allocates them, the results and -- when none is passed -- the workspace."""
    if pieces is not None and len(pieces) != len(desc_in):
        raise HipError("pcm_decimate: %d pieces for %d streams" % (len(pieces), len(desc_in)))
    return _writer_call("pcm_decimate", "dvda_pcm_hip_decimate", "the decimation", DecimReport, d_in, layout_in, desc_in,
                        None if pieces is None else lambda: _piece_records(pieces), (ratio, bits), out, layout_out, desc_out,
                        lambda: decim_desc_out(desc_in, ratio, pieces), False, max_total_out_frames, work)


def pcm_decimate_workspace_words(n, max_total_out_frames):
    """dvda_pcm_hip_decimate_workspace_words: the uint32 words of workspace pcm_decimate needs for n streams whose
    OUTPUT frames sum to at most max_total_out_frames (what `work` must hold when the caller passes one); needs no GPU"""
    return int(lib().dvda_pcm_hip_decimate_workspace_words(n, max_total_out_frames))


def decim_list(d_report):
    """pcm_decimate's report tensor -> list of DecimReport.as_dict() on the host (waits)"""
    return _record_list(DecimReport, d_report)


def resample_taps():
    """dvda_pcm_hip_resample_taps: the committed table g[147][96] as an int32 array (a copy); needs no GPU"""
    ph, tp = ctypes.c_uint32(0), ctypes.c_uint32(0)
    p = lib().dvda_pcm_hip_resample_taps(ctypes.byref(ph), ctypes.byref(tp))
    return np.ctypeslib.as_array(p, (int(ph.value), int(tp.value))).astype(np.int32)


def resample_out_frames(frame0, own):
    """dvda_pcm_hip_resample_out_frames: output frames of the absolute frames [frame0, frame0 + own); needs no GPU"""
    return int(lib().dvda_pcm_hip_resample_out_frames(frame0, own))


def resample_value(window, phase, bits):
    """dvda_pcm_hip_resample_value: one output value of phase `phase` from its window of 96 input values -> (value, 1 when
    the clamp changed it else 0); host arithmetic, needs no GPU.  HipError for an invalid phase or depth or a window of
    another length"""
    w = np.ascontiguousarray(window, np.int32)
    if w.shape != (RSM_TAPS,):
        raise HipError("dvda_pcm_hip_resample_value: a window of %s values" % (w.shape,))
    return _value_call("dvda_pcm_hip_resample_value", "(phase %r, bits %r)" % (phase, bits), w.ctypes.data, phase, bits)


def resample_desc_out(desc_in, pieces=None):
    """the output descriptors pcm_resample makes when none are passed, as decim_desc_out -> (desc_out, words)"""
    def shape(i, frames, ch, ok):
        frame0, before, after = pieces[i] if pieces is not None else (0, 0, 0)
        return (resample_out_frames(frame0, frames - before - after) if ok and before + after <= frames else 0), ch
    return _end_to_end(desc_in, shape)


def pcm_resample(d_in, layout_in, desc_in, bits, pieces=None, out=None, layout_out=None, desc_out=None,
                 max_total_out_frames=None, work=None):
    """dvda_pcm_hip_resample over torch tensors, with pcm_decimate's shapes: d_in an int32 tensor on the device holding
    the streams in layout_in (PCM_PLANAR or PCM_INTERLEAVED), desc_in a list of (off, stride, frames, channels); every
    stream taken as 48 kHz and resampled to 44.1 kHz, the values clamped to `bits`.  pieces: per stream (frame0, before,
    after) (None: whole tracks).  out / layout_out / desc_out: where the result goes -- default: the input's layout, the
    regions end to end in a fresh zeroed tensor (resample_desc_out).  -> (d_out, desc_out, d_report): the output tensor,
    its descriptors and a uint8 device tensor [n, sizeof(DecimReport)] (decim_list brings it to the host).  Only the
    kernels are asynchronous, on torch's current stream."""
    if pieces is not None and len(pieces) != len(desc_in):
        raise HipError("pcm_resample: %d pieces for %d streams" % (len(pieces), len(desc_in)))
    return _writer_call("pcm_resample", "dvda_pcm_hip_resample", "the resampler", DecimReport, d_in, layout_in, desc_in,
                        None if pieces is None else lambda: _piece_records(pieces), (bits,), out, layout_out, desc_out,
                        lambda: resample_desc_out(desc_in, pieces), False, max_total_out_frames, work)


def pcm_resample_workspace_words(n, max_total_out_frames):
    """dvda_pcm_hip_resample_workspace_words: the uint32 words of workspace pcm_resample needs for n streams whose
    OUTPUT frames sum to at most max_total_out_frames; needs no GPU"""
    return int(lib().dvda_pcm_hip_resample_workspace_words(n, max_total_out_frames))


def _mix_record(m):
    """a PcmMix, or the dict PcmMix.as_dict() gives -> a PcmMix"""
    return m if isinstance(m, PcmMix) else PcmMix.from_dict(m)


def speaker_mask(assignment):
    """dvda_pcm_hip_speaker_mask: the RIFF-WAVE speaker mask of DVD-Audio channel assignment 0..20, else 0; needs no GPU"""
    return int(lib().dvda_pcm_hip_speaker_mask(assignment))


def mix_matrix(mask, out_channels=2, flags=MIX_NORMALIZED):
    """dvda_pcm_hip_mix_matrix: the default matrix of a buffer whose channel c is the c-th set bit of `mask`, to 1 or 2
    channels -> PcmMix.as_dict(); host arithmetic, needs no GPU.  HipError (EINVAL) for a mask, a channel count or flags
    the call does not take"""
    rec = PcmMix()
    _check(lib().dvda_pcm_hip_mix_matrix(mask, out_channels, flags, ctypes.byref(rec)), "dvda_pcm_hip_mix_matrix")
    return rec.as_dict()


def mix_valid(m):
    """dvda_pcm_hip_mix_valid: whether the kernels take the matrix; needs no GPU"""
    return bool(lib().dvda_pcm_hip_mix_valid(ctypes.byref(_mix_record(m))))


def mix_value(x, m, o, bits):
    """dvda_pcm_hip_mix_value: output channel o of the frame whose in_channels values are x -> (value, 1 when the clamp
    changed it else 0); host arithmetic, needs no GPU.  HipError for an invalid matrix, channel or depth or another
    number of values"""
    rec = _mix_record(m)
    v = np.ascontiguousarray(x, np.int32)
    if v.shape != (int(rec.in_channels),):
        raise HipError("dvda_pcm_hip_mix_value: %s values for %d channels" % (v.shape, rec.in_channels))
    return _value_call("dvda_pcm_hip_mix_value", "(channel %r, bits %r)" % (o, bits), v.ctypes.data, ctypes.byref(rec), o, bits)


def _mix_records(matrices):
    """a list of matrices -> their dvda_pcm_mix records as a numpy array of bytes rows (one at least)"""
    rec = np.zeros((max(len(matrices), 1), ctypes.sizeof(PcmMix)), np.uint8)
    for i, m in enumerate(matrices):
        rec[i] = np.frombuffer(bytes(_mix_record(m)), np.uint8)
    return rec


def mix_desc_out(desc_in, matrices):
    """the output descriptors pcm_mix makes when none are passed: per stream the input's frames and the matrix's output
    channels, the regions end to end with the stride = the frames, which serves either int32 layout -> (desc_out, words)"""
    och = [int(_mix_record(m).out_channels) for m in matrices]
    return _end_to_end(desc_in[:len(och)], lambda i, frames, ch, ok: (frames if ok and 1 <= och[i] <= 8 else 0, och[i]))


def pcm_mix(d_in, layout_in, desc_in, matrices, bits, out=None, layout_out=None, desc_out=None, max_total_frames=None,
            work=None):
    """dvda_pcm_hip_mix over torch tensors: d_in an int32 tensor on the device holding the streams in layout_in
    (PCM_PLANAR or PCM_INTERLEAVED), desc_in a list of (off, stride, frames, channels), matrices one PcmMix (or its dict)
    per stream; every stream mixed through its matrix, the values clamped to `bits`.  out / layout_out / desc_out: where
    the result goes -- default: the input's layout, the regions end to end in a fresh zeroed tensor (mix_desc_out).  ->
    (d_out, desc_out, d_report): the output tensor, its descriptors and a uint8 device tensor [n, sizeof(PcmMixReport)]
    (mix_list brings it to the host).  Only the kernels are asynchronous, on torch's current stream: like pcm_levels, this
    helper builds the descriptors and matrices on the host, copies them to the device and allocates them, the results
    and -- when none is passed -- the workspace."""
    if len(matrices) != len(desc_in):
        raise HipError("pcm_mix: %d matrices for %d streams" % (len(matrices), len(desc_in)))
    return _writer_call("pcm_mix", "dvda_pcm_hip_mix", "the channel mix", PcmMixReport, d_in, layout_in, desc_in,
                        lambda: _mix_records(matrices), (bits,), out, layout_out, desc_out,
                        lambda: mix_desc_out(desc_in, matrices), True, max_total_frames, work)


def pcm_mix_workspace_words(n, max_total_frames):
    """dvda_pcm_hip_mix_workspace_words: the uint32 words of workspace pcm_mix needs for n streams whose frames sum to at
    most max_total_frames; needs no GPU"""
    return int(lib().dvda_pcm_hip_mix_workspace_words(n, max_total_frames))


def mix_list(d_report):
    """pcm_mix's report tensor -> list of PcmMixReport.as_dict() on the host (waits)"""
    return _record_list(PcmMixReport, d_report)


def crc_list(d_crc, d_nbytes):
    """pcm_crc32's tensors -> list of (crc, nbytes) on the host (waits)"""
    c = d_crc.cpu().numpy().view(np.uint32)
    b = d_nbytes.cpu().numpy()
    return [(int(x), int(y)) for x, y in zip(c, b)]


ROWS_PER_AU = {0: 40, 8: 40, 1: 80, 9: 80, 2: 160, 10: 160}


def pack_streams(streams):
    """list of uint8 arrays -> (flat uint8 array with 64 spare bytes, offsets, lengths); 16-byte aligned"""
    offs, lens, pos = [], [], 0
    for s in streams:
        offs.append(pos)
        lens.append(len(s))
        pos += (len(s) + 15) & ~15
    flat = np.zeros(pos + 64, np.uint8)
    for s, o in zip(streams, offs):
        flat[o:o + len(s)] = s
    return flat, np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)


def _cuda(device, what):
    import torch
    if not torch.cuda.is_available():
        raise HipError("no GPU visible to torch: the %s path is HIP-only" % what)
    return torch.device("cuda", device)


class Batch:
    """The input side of a decode on the device: the packed bytes (d_bytes, `total` of them in front of 64 spare ones)
    and the n streams' ranges in them (d_off, d_len) -- what Context.index_batch reads.  The tensors must live as long
    as an index of them is decoded: index_batch keeps the batch for that; a caller of the pointer-level index() keeps it."""

    def __init__(self, streams=None, device=0, packed=None):
        """packed: (flat, offs, lens) of bytes that are packed already (pack_streams, synth.batch), with any ranges in them"""
        import torch
        flat, offs, lens = pack_streams(streams) if packed is None else packed
        self.dev = _cuda(device, "MLP decode")
        self.d_bytes = torch.from_numpy(flat).to(self.dev)
        self.total = int(len(flat) - 64)
        self._ranges(offs, lens)

    def _ranges(self, offs, lens):
        import torch
        self.d_off = torch.from_numpy(np.asarray(offs, np.int64)).to(self.dev)
        self.d_len = torch.from_numpy(np.asarray(lens, np.int64)).to(self.dev)
        self.n = len(self.d_off)

    def with_ranges(self, offs, lens):
        """the same bytes on the device under other ranges (the index checks ranges, it does not trust them)"""
        import copy
        other = copy.copy(self)
        other._ranges(offs, lens)
        return other

    @property
    def current_stream(self):
        """torch's current stream on the batch's device (not a stream of the batch's own), as the C ABI takes it"""
        import torch
        return torch.cuda.current_stream(self.dev).cuda_stream


def standard_rows(info):
    """PCM frames a stream decodes to when every access unit has the standard length of its rate"""
    return int(info.mlp_frames) * ROWS_PER_AU.get(int(info.group0_rate), 0)


def grown_rows(rows, infos):
    """the capacities a decode that reported DVDA_ST_OVERFLOW asks for: pcm_frames where that is more than the stream has"""
    return [max(int(r), int(inf.pcm_frames)) for r, inf in zip(rows, infos)]


def sample_bytes(layout):
    return {PCM_WAV24: 3, PCM_WAV16: 2}.get(layout, 4)


def region_words(rows, channels, layout):
    """int32 words of one stream's output region: the values themselves, or the WAV payload rounded up to words plus
    four, so that every stream starts dword-aligned with room for the kernels' whole-word stores"""
    nb = sample_bytes(layout)
    return rows * channels if nb == 4 else (rows * channels * nb + 3) // 4 + 4


def region_layout(rows, channels, layout):
    """-> (out_off[i] in int32 words, words of the buffer: at least 1) for regions laid end to end"""
    out_off, pos = [], 0
    for r, c in zip(rows, channels):
        out_off.append(pos)
        pos += region_words(r, c, layout)
    return out_off, max(pos, 1)


def cut_regions(host, out_off, rows, channels, frames, layout):
    """a host copy of the PCM buffer (int32) -> per stream int32 [channels, min(frames, rows)] for PCM_PLANAR /
    PCM_INTERLEAVED, the payload bytes (uint8) of that many frames for PCM_WAV24 / PCM_WAV16"""
    nb = sample_bytes(layout)
    pcm = []
    for o, r, c, f in zip(out_off, rows, channels, frames):
        f = min(int(f), r)
        if nb != 4:
            pcm.append(host.view(np.uint8)[4 * o:4 * o + f * c * nb].copy())
        elif not r * c:
            pcm.append(np.zeros((c, 0), np.int32))
        elif layout == PCM_INTERLEAVED:
            pcm.append(np.ascontiguousarray(host[o:o + r * c].reshape(r, c).T[:, :f]))
        else:
            pcm.append(np.ascontiguousarray(host[o:o + r * c].reshape(c, r)[:, :f]))
    return pcm


class PcmRegions:
    """The output side of a decode on the device: d_pcm and, per stream, where its region starts (d_out_off, int32
    words) and its capacity in PCM frames (d_stride = rows).  Regions lie end to end unless the caller places them
    (out_off); the buffer ends `slack` words behind the last region and starts out filled with `fill` (None: as
    allocated)."""

    def __init__(self, rows, channels, layout=PCM_PLANAR, device=0, out_off=None, slack=0, fill=0):
        import torch
        self.dev = _cuda(device, "MLP decode")
        self.rows, self.channels, self.layout = [int(r) for r in rows], [int(c) for c in channels], layout
        self.out_off, words = region_layout(self.rows, self.channels, layout)
        if out_off is not None:
            self.out_off = [int(o) for o in out_off]
            words = max([o + region_words(r, c, layout) for o, r, c in zip(self.out_off, self.rows, self.channels)] + [1])
        if fill is None:
            self.d_pcm = torch.empty(words + slack, dtype=torch.int32, device=self.dev)
        else:
            self.d_pcm = torch.full((words + slack,), fill, dtype=torch.int32, device=self.dev)
        self.d_out_off = torch.tensor(self.out_off, dtype=torch.int64, device=self.dev)
        self.d_stride = torch.tensor(self.rows, dtype=torch.int64, device=self.dev)

    @classmethod
    def for_infos(cls, infos, layout=PCM_PLANAR, device=0, **kw):
        """regions of standard length for the streams of an index"""
        return cls([standard_rows(inf) for inf in infos], [int(inf.channels) for inf in infos], layout, device, **kw)

    def grown(self, infos):
        """new regions with room for what the decode behind `infos` asked for (grown_rows)"""
        return PcmRegions(grown_rows(self.rows, infos), self.channels, self.layout, self.dev.index)

    @property
    def ptrs(self):
        """(d_pcm, d_out_off, d_out_stride) as Context.decode, decode_async and pcm_crc32 take them"""
        return self.d_pcm.data_ptr(), self.d_out_off.data_ptr(), self.d_stride.data_ptr()

    def to_host(self, infos):
        """copies the buffer back (waits) and cuts it at the streams' pcm_frames (cut_regions)"""
        return cut_regions(self.d_pcm.cpu().numpy(), self.out_off, self.rows, self.channels,
                           [inf.pcm_frames for inf in infos], self.layout)


def decode_batch(ctx, batch, layout, attempts=1, capacity="report", decode=Context.decode, crc_bits=None, stream=None,
                 levels=None, to_host=True, energy=None):
    """The decode sequence, once: index; regions of standard length in `layout` (what ctx is set to); up to `attempts`
    rounds of decode, each after the first on regions grown to what DVDA_ST_OVERFLOW asked for and a new index; the
    digest at crc_bits if given; the host copy.  -> (pcm as cut_regions gives it, infos, digests or None)
    levels: a bit depth -- the level report at that depth too (Context.pcm_levels), appended: -> (pcm, infos, digests or
    None, reports)
    energy: a block length -- the energy report on that grid too (Context.pcm_energy), appended behind whatever `levels`
    appended (with energy alone: -> (pcm, infos, digests or None, blocks)): one list of blocks per stream
    capacity: what more major syncs than the context holds (sync patterns in payload count too) lead to -- "report":
    DVDA_ST_CAPACITY on the streams; "raise": HipError; a function: called with the count the index found, it returns
    the larger context the sequence goes on with (the caller's to close).
    decode: Context.decode or Context.decode_async.  stream: default torch's current one on the batch's device.
    to_host=False: no host copy -- the first element is the PcmRegions the last round decoded into, on the device."""
    st = batch.current_stream if stream is None else stream
    ctx.index_batch(batch, st)
    if capacity != "report":
        try:
            ctx.segment_count(st)
        except HipError:
            if capacity == "raise":
                raise
            found = ctypes.c_uint32()
            lib().dvda_mlp_hip_segment_count(ctx._h, ctypes.byref(found), st)
            ctx = capacity(int(found.value))
            ctx.index_batch(batch, st)
    infos = ctx.stream_info(stream=st)
    regions = PcmRegions.for_infos(infos, layout, ctx.device)
    for attempt in range(attempts):
        if attempt:
            regions = regions.grown(infos)
            ctx.index_batch(batch, st)
        decode(ctx, *regions.ptrs, st)
        infos = ctx.stream_info(stream=st)
        if not any(inf.status & ST["OVERFLOW"] for inf in infos):
            break
    digests = ctx.pcm_crc32(*regions.ptrs, crc_bits, stream=st) if crc_bits else None
    pcm = regions.to_host(infos) if to_host else regions
    more = ()
    if levels is not None:
        more += (ctx.pcm_levels(*regions.ptrs, levels, stream=st),)
    if energy:
        more += (ctx.pcm_energy(*regions.ptrs, energy, stream=st),)
    return (pcm, list(infos), digests) + more


def _context_for(ctx, batch, max_segments, lanes_per_segment, layout):
    """-> (the caller's context set to this call's lanes and layout, or a context of the call's own; is it the call's own)"""
    if ctx is None:
        segments = max(64, batch.total // 64) if max_segments is None else max_segments
        return Context(batch.dev.index, batch.n, segments, lanes_per_segment, layout), True
    ctx.set_lanes_per_segment(lanes_per_segment)
    ctx.set_pcm_layout(layout)
    return ctx, False


@contextlib.contextmanager
def _call_context(ctx, batch, max_segments, lanes_per_segment, layout, presentation):
    """The context a decode_streams* call runs on, for a `with`: the caller's, set to this call's lanes, layout and
    presentation, or one of the call's own, which the decode sequence may replace by a larger one and which is closed when
    the block ends, however it ends.  -> (ctx, capacity) as decode_batch takes them."""
    ctx, own = _context_for(ctx, batch, max_segments, lanes_per_segment, layout)
    made = [ctx]

    def larger(found):
        made[0].close()
        made[0] = Context(batch.dev.index, batch.n, found + 64, lanes_per_segment, layout)
        if presentation != PRESENT_FULL:
            made[0].set_presentation(presentation)
        return made[0]

    try:
        if presentation != PRESENT_FULL or not own:
            ctx.set_presentation(presentation)
        yield ctx, larger if own else "raise"
    finally:
        if own:
            made[0].close()


def _decoded_lists(infos, regions):
    """what the passes behind a decode need of it, per stream -> (frames: those its region holds, 0 for a stream with
    DVDA_ST_OVERFLOW; desc: (off, stride, frames, channels); depth: its bits, 0 for a code that has none)"""
    frames = [0 if inf.status & ST["OVERFLOW"] else min(int(inf.pcm_frames), r) for inf, r in zip(infos, regions.rows)]
    desc = [(o, r, f, c) for o, r, f, c in zip(regions.out_off, regions.rows, frames, regions.channels)]
    return frames, desc, [BITS_OF_CODE.get(int(inf.group0_bps), 0) for inf in infos]


def decode_streams(streams, device=0, max_segments=None, lanes_per_segment=0, layout=PCM_PLANAR, ctx=None,
                   presentation=PRESENT_FULL, crc32=False, crc_bits=24, levels=None, energy=None):
    """Decodes a list of complete MLP byte streams on the GPU.

    Returns (pcm, infos): pcm[i] is an int32 array [channels, pcm_frames] in RIFF-WAVE
    channel order -- what the reference appends to `samples` (src/mlp.c:527-533) --
    and infos[i] the dvda_mlp_stream_info of stream i.  With layout=PCM_INTERLEAVED the
    library writes frame-major (the dvda_read order) and pcm[i] is that buffer viewed
    as [pcm_frames, channels] and transposed, so callers compare the same way.  Raises
    HipError if the HIP path is unavailable; never falls back to a CPU decoder.
    `ctx`: a caller's Context to run on (it stays open and keeps its size: a batch it cannot hold raises); its lane,
    layout and presentation settings are set to this call's.  A context of the call's own grows to the batch.
    presentation=PRESENT_SUBSTREAM0: two-substream streams come out as the k-channel presentation of substream 0
    (pcm[i] is [k, pcm_frames], infos[i].channels == k); one-substream streams as always.
    crc32=True: -> (pcm, infos, digests), digests[i] = (zlib CRC-32 of stream i's WAV payload at crc_bits, its bytes),
    computed on the device from the PCM where the decode wrote it (Context.pcm_crc32).
    levels=<bits> (16, 20 or 24): the level report of every stream at that nominal depth (Context.pcm_levels) is appended
    to the result: -> (pcm, infos, reports) or (pcm, infos, digests, reports).  layout must be an int32 one.
    energy=<block_frames> (64 .. 2^24): the energy report of every stream on that block grid (Context.pcm_energy), one
    list of blocks per stream, is appended behind all of the above.  layout must be an int32 one.
    """
    batch = Batch(streams, device)
    with _call_context(ctx, batch, max_segments, lanes_per_segment, layout, presentation) as (ctx, capacity):
        # (int32 regions of r*c words, cut as [c, r], for any layout but PCM_INTERLEAVED)
        res = decode_batch(ctx, batch, layout if layout == PCM_INTERLEAVED else PCM_PLANAR, attempts=2, capacity=capacity,
                           crc_bits=crc_bits if crc32 else None, levels=levels, energy=energy)
        pcm, infos, digests = res[:3]
        return ((pcm, infos, digests) if crc32 else (pcm, infos)) + tuple(res[3:])


def decode_streams_concealed(streams, device=0, max_segments=None, lanes_per_segment=0, layout=PCM_PLANAR, init_fir=None,
                             crc32=False, crc_bits=24, ctx=None, levels=None, energy=None):
    """decode_streams in conceal mode (dvda_mlp_hip_set_conceal): a damaged stream comes out as kept PCM ++ silence ++
    PCM of a fresh decoder ++ ... instead of a non-benign status (include/dvda_mlp_hip.h states the rule).

    -> (pcm, infos, spans).  pcm[i] as decode_streams gives it (int32 [channels, pcm_frames]) for PCM_PLANAR /
    PCM_INTERLEAVED, the payload bytes (uint8) for PCM_WAV24 / PCM_WAV16; spans[i] = list of
    (first_frame, frames, byte_off, byte_end, cause, flags), empty for a stream without damage.
    init_fir: optional int32 [n_streams, 2, 48], the FIR history the streams start with (dvda_mlp_hip_set_initial_fir).
    crc32=True: -> (pcm, infos, spans, digests): (CRC-32, bytes) of every stream's WAV payload as it was handed out, at the
    depth of the WAV layout or at crc_bits for the int32 layouts (Context.pcm_crc32).
    levels=<bits>: the level report of every stream as it was handed out -- the concealed gaps are exact zeros -- is
    appended to the result (Context.pcm_levels; HipError for a WAV layout).
    energy=<block_frames>: the energy report of every stream as it was handed out, behind that (Context.pcm_energy).
    `ctx`: a caller's Context to run on: its lane and layout settings are set to this call's, its presentation to
    PRESENT_FULL; conceal mode (and init_fir) are taken off it again when the call ends, however it ends.  It keeps its
    size: a batch it cannot hold raises."""
    import torch
    batch = Batch(streams, device)
    ctx, own = _context_for(ctx, batch, max_segments, lanes_per_segment, layout)
    d_fir, done = None, False
    try:
        if not own:
            ctx.set_presentation(PRESENT_FULL)
        ctx.set_conceal(True)           # (before the index)
        if init_fir is not None:
            d_fir = torch.from_numpy(np.ascontiguousarray(init_fir, np.int32).reshape(batch.n, 2, 48)).to(batch.dev)
            ctx.set_initial_fir(d_fir.data_ptr())
        # silence and a fresh decoder's access units can need more than the index's count, and then once more
        res = decode_batch(ctx, batch, layout, attempts=3, capacity="report" if own else "raise",
                           crc_bits={PCM_WAV24: 24, PCM_WAV16: 16}.get(layout, crc_bits) if crc32 else None, levels=levels,
                           energy=energy)
        pcm, infos, digests = res[:3]
        spans = [ctx.conceal_spans(i, batch.current_stream) for i in range(batch.n)]
        done = True
        return ((pcm, infos, spans, digests) if crc32 else (pcm, infos, spans)) + tuple(res[3:])
    finally:
        if own:
            ctx.close()
        else:
            rc = lib().dvda_mlp_hip_set_conceal(ctx._h, 0)
            if d_fir is not None:
                rc = rc or lib().dvda_mlp_hip_set_initial_fir(ctx._h, None)
            if done:                    # (a call that failed reports its own error, not this one)
                _check(rc, "leaving conceal mode")


def compare_streams(streams_a, streams_b, device=0, layout_a=PCM_INTERLEAVED, layout_b=PCM_INTERLEAVED, bits=0,
                    conceal=False):
    """Two rips of the same titles: decodes both lists of complete MLP byte streams (the one decode sequence,
    decode_batch, each batch on a context of its own, in layout_a / layout_b; conceal=True: both in conceal mode) and
    compares stream i of A with stream i of B where the decodes wrote them (Context.pcm_compare) -- no PCM is copied to
    the host.  -> (infos_a, infos_b, diffs), diffs[i] a Diff.as_dict().  bits as pcm_compare takes it.  A stream whose
    region the decode could not fill (DVDA_ST_OVERFLOW after the sequence's attempts) is an empty side."""
    if len(streams_a) != len(streams_b):
        raise HipError("compare_streams: %d streams against %d" % (len(streams_a), len(streams_b)))
    sides = []
    try:
        for streams, layout in ((streams_a, layout_a), (streams_b, layout_b)):
            if layout not in (PCM_PLANAR, PCM_INTERLEAVED):
                raise HipError("compare_streams: the compare takes the int32 layouts only (EINVAL)")
            batch = Batch(streams, device)
            ctx, _ = _context_for(None, batch, None, 0, layout)
            sides.append((ctx, batch))
            if conceal:
                ctx.set_conceal(True)       # (before the index)
            regions, infos, _ = decode_batch(ctx, batch, layout, attempts=3 if conceal else 2, to_host=False)
            sides[-1] = (ctx, batch, regions, infos)
        (ctx_a, batch_a, reg_a, infos_a), (_, _, reg_b, infos_b) = sides
        desc_b = [(o, r, 0 if inf.status & ST["OVERFLOW"] else int(inf.pcm_frames), int(inf.channels))
                  for o, r, inf in zip(reg_b.out_off, reg_b.rows, infos_b)]
        diffs = ctx_a.pcm_compare(*reg_a.ptrs, reg_b.d_pcm, layout_b, desc_b, bits, stream=batch_a.current_stream)
        return infos_a, infos_b, diffs
    finally:
        for side in sides:
            side[0].close()


def shard_c(sizes, parts):
    """dvda_mlp_hip_shard: the C restatement of shard.shard_titles -> owner[i]"""
    import numpy as np
    sz = np.ascontiguousarray(sizes, np.uint64)
    out = np.zeros(len(sz), np.uint32)
    _check(lib().dvda_mlp_hip_shard(sz.ctypes.data, len(sz), parts, out.ctypes.data), "dvda_mlp_hip_shard")
    return out


def decode_streams_multi(streams, devices, layout=PCM_PLANAR, max_segments=None):
    """dvda_mlp_hip_decode_multi: host streams dealt to the device entries of `devices` (a device may be named more
    than once), host PCM back.  -> (pcm list as decode_streams gives it, infos, MultiSummary)"""
    import numpy as np
    n = len(streams)
    bufs = [np.ascontiguousarray(s, np.uint8) for s in streams]
    lens = np.array([len(b) for b in bufs], np.uint64)
    if max_segments is None:
        max_segments = int(sum(len(b) // 2048 + 8 for b in bufs))
    devs = np.array(devices, np.int32)
    h = ctypes.c_void_p()
    _check(lib().dvda_mlp_hip_create_multi(ctypes.byref(h), devs.ctypes.data, len(devs), n, max_segments),
           "dvda_mlp_hip_create_multi")
    try:
        vb = 3 if layout == PCM_WAV24 else 2 if layout == PCM_WAV16 else 4
        caps = np.array([len(b) + 4096 for b in bufs], np.uint64)      # PCM frames: a frame takes more than a byte
        outs = [np.zeros(int(c) * 6 * vb + 16, np.uint8) for c in caps]
        sp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
        op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        infos = (StreamInfo * n)()
        summ = MultiSummary()
        _check(lib().dvda_mlp_hip_decode_multi(h, sp, lens.ctypes.data, n, layout, op, caps.ctypes.data, infos,
                                               ctypes.byref(summ)), "dvda_mlp_hip_decode_multi")
        pcm = []
        for i in range(n):
            f, ch, cap = int(infos[i].pcm_frames), int(infos[i].channels), int(caps[i])
            f = min(f, cap)
            if layout == PCM_PLANAR:
                pcm.append(outs[i][:cap * ch * 4].view(np.int32).reshape(ch, cap)[:, :f].copy() if ch else np.zeros((0, 0), np.int32))
            elif layout == PCM_INTERLEAVED:
                pcm.append(outs[i][:f * ch * 4].view(np.int32).reshape(f, ch).T.copy() if ch else np.zeros((0, 0), np.int32))
            else:
                pcm.append(outs[i][:f * ch * vb].copy())
        return pcm, list(infos), summ
    finally:
        lib().dvda_mlp_hip_destroy_multi(h)


def decode_streams_wav(streams, bits, device=0, lanes_per_segment=0, presentation=PRESENT_FULL, crc32=False):
    """Decodes complete MLP byte streams straight into the interleaved little-endian WAV payload dvda2wav
    writes (DVDA_PCM_WAV24 / DVDA_PCM_WAV16: the output stage fused into the decode kernels).
    -> (list of uint8 arrays, infos); crc32=True: -> (payloads, infos, digests), digests[i] = (CRC-32, bytes) of payload i
    computed on the device (Context.pcm_crc32)."""
    batch = Batch(streams, device)
    assert bits in (16, 24)
    layout = PCM_WAV24 if bits == 24 else PCM_WAV16
    ctx, _ = _context_for(None, batch, None, lanes_per_segment, layout)
    try:
        if presentation != PRESENT_FULL:
            ctx.set_presentation(presentation)
        out, infos, digests = decode_batch(ctx, batch, layout, attempts=2, crc_bits=bits if crc32 else None)
        return (out, infos, digests) if crc32 else (out, infos)
    finally:
        ctx.close()


BITS_OF_CODE = {0: 16, 1: 20, 2: 24}      # the major sync's group-0 depth code


def decode_streams_requantized(streams, bits_out, mode=RQ_TPDF, seed=0, device=0, layout=PCM_PLANAR, wav=False, ctx=None,
                               presentation=PRESENT_FULL):
    """Decodes complete MLP byte streams and reduces them to bits_out bits on the device (pcm_requantize: truncated,
    rounded or dithered with `seed`, clamped), each from its own depth; streams of different depths run as one call per
    depth.  -> (pcm, infos, reports): pcm[i] as decode_streams gives it (layout: PCM_PLANAR or PCM_INTERLEAVED), or with
    wav=True (bits_out 16 or 24) the WAV payload as a uint8 array; reports[i] = RequantReport.as_dict().  A stream whose
    depth is below bits_out comes out as decoded, reports[i] = None (wav=True: its payload at its own depth)."""
    import torch
    if layout not in (PCM_PLANAR, PCM_INTERLEAVED) or (wav and bits_out not in (16, 24)):
        raise HipError("decode_streams_requantized: EINVAL (an int32 layout; a payload has 16 or 24 bits)")
    batch = Batch(streams, device)
    with _call_context(ctx, batch, None, 0, layout, presentation) as (ctx, capacity):
        regions, infos, _ = decode_batch(ctx, batch, layout, attempts=2, capacity=capacity, to_host=False)
    n = len(infos)
    frames, desc, depth = _decoded_lists(infos, regions)
    wav_layout = PCM_WAV24 if bits_out == 24 else PCM_WAV16
    d_wav = w_off = None
    if wav:
        w_off, words = region_layout(regions.rows, regions.channels, wav_layout)
        d_wav = torch.zeros(words, dtype=torch.int32, device=regions.dev)
    reports = [None] * n
    for bits_in in sorted(set(depth)):
        idx = [i for i in range(n) if depth[i] == bits_in and bits_in >= bits_out]
        if not idx:
            continue
        sub = [desc[i] for i in idx]
        if wav:
            sub_out = [(w_off[i],) + desc[i][1:] for i in idx]
            _, d_rep = pcm_requantize(regions.d_pcm, layout, sub, bits_in, bits_out, mode, seed, out=d_wav,
                                      layout_out=wav_layout, desc_out=sub_out)
        else:
            _, d_rep = pcm_requantize(regions.d_pcm, layout, sub, bits_in, bits_out, mode, seed, out=regions.d_pcm)
        for i, rep in zip(idx, requant_list(d_rep)):
            reports[i] = rep
    pcm = regions.to_host(infos)
    if wav:
        pay = cut_regions(d_wav.cpu().numpy(), w_off, regions.rows, regions.channels, frames, wav_layout)
        for i in range(n):
            if reports[i] is not None:
                pcm[i] = pay[i]
            elif depth[i] in (16, 24):      # as decoded: write_signed at its own depth
                v = np.ascontiguousarray(pcm[i].T).reshape(-1).astype(np.int64)
                w = (v & ((1 << (depth[i] - 1)) - 1)) | np.where(v < 0, 1 << (depth[i] - 1), 0)
                pcm[i] = np.stack([(w >> (8 * k)) & 0xFF for k in range(depth[i] // 8)], 1).astype(np.uint8).reshape(-1)
            else:
                raise HipError("decode_streams_requantized: stream %d has %d bits: no WAV payload" % (i, depth[i]))
    return pcm, list(infos), reports


RATE_OF_CODE = {0: 48000, 1: 96000, 2: 192000, 8: 44100, 9: 88200, 10: 176400}    # the major sync's group-0 rate code


def decode_streams_decimated(streams, ratio, device=0, layout=PCM_PLANAR, ctx=None, presentation=PRESENT_FULL):
    """Decodes complete MLP byte streams and decimates them by `ratio` (2 or 4) on the device (pcm_decimate), each
    clamped at its own depth; streams of different depths run as one call per depth.  -> (pcm, rates, infos, reports):
    pcm[i] int32 [channels, ceil(frames / ratio)] as decode_streams gives it, rates[i] the new rate in Hz, reports[i] =
    DecimReport.as_dict().  ValueError when a stream's rate / ratio is not 44 100, 48 000, 88 200 or 96 000 Hz: judged
    from the index's stream records, before anything is decoded.  A stream
    whose region the decode could not fill (DVDA_ST_OVERFLOW) comes out empty with a report of zeros."""
    if layout not in (PCM_PLANAR, PCM_INTERLEAVED) or ratio not in (2, 4):
        raise HipError("decode_streams_decimated: EINVAL (an int32 layout, a ratio of 2 or 4)")
    batch = Batch(streams, device)
    rates = []

    def decode(c, *args):
        # the rates are the index's: a batch that cannot be divided costs no decode
        del rates[:]
        for i, inf in enumerate(c.stream_info(stream=args[-1])):
            rate = RATE_OF_CODE.get(int(inf.group0_rate), 0)
            if rate % ratio or rate // ratio not in DECIM_RATES:
                raise ValueError("decode_streams_decimated: stream %d runs at %d Hz: no %d Hz output" % (i, rate, rate // ratio))
            rates.append(rate // ratio)
        return Context.decode(c, *args)

    with _call_context(ctx, batch, None, 0, layout, presentation) as (ctx, capacity):
        regions, infos, _ = decode_batch(ctx, batch, layout, attempts=2, capacity=capacity, decode=decode, to_host=False)
    n = len(infos)
    _, desc, depth = _decoded_lists(infos, regions)
    desc_out, words = decim_desc_out(desc, ratio)
    import torch
    d_out = torch.zeros(words, dtype=torch.int32, device=regions.dev)
    reports = [None] * n
    for bits in sorted(set(depth)):
        idx = [i for i in range(n) if depth[i] == bits]
        _, _, d_rep = pcm_decimate(regions.d_pcm, layout, [desc[i] for i in idx], ratio, bits, out=d_out, layout_out=layout,
                                   desc_out=[desc_out[i] for i in idx])
        for i, rep in zip(idx, decim_list(d_rep)):
            reports[i] = rep
    pcm = cut_regions(d_out.cpu().numpy(), [d[0] for d in desc_out], [d[1] for d in desc_out], regions.channels,
                      [d[2] for d in desc_out], layout)
    return pcm, rates, list(infos), reports


def decode_streams_resampled(streams, rate=RESAMPLE_RATE, device=0, layout=PCM_PLANAR, ctx=None, presentation=PRESENT_FULL):
    """Decodes complete MLP byte streams and brings each to `rate` = 44 100 Hz on the device, by its own rate: 44.1 kHz as
    it is; 88.2 / 176.4 kHz decimated by 2 / 4 (pcm_decimate); 48 kHz resampled (pcm_resample); 96 / 192 kHz decimated
    by 2 / 4 into an intermediate buffer at the stream's depth, then resampled -- by definition the composition of the
    two passes.  Each stream is clamped at its own depth.  -> (pcm, infos, reports): pcm[i] int32 [channels, frames at
    44.1 kHz], reports[i] = dict(decimate=DecimReport.as_dict() or None, resample=DecimReport.as_dict() or None).
    ValueError for any other `rate`."""
    if rate != RESAMPLE_RATE:
        raise ValueError("decode_streams_resampled: %r Hz: only %d Hz is made" % (rate, RESAMPLE_RATE))
    if layout not in (PCM_PLANAR, PCM_INTERLEAVED):
        raise HipError("decode_streams_resampled: EINVAL (an int32 layout)")
    import torch
    batch = Batch(streams, device)
    with _call_context(ctx, batch, None, 0, layout, presentation) as (ctx, capacity):
        regions, infos, _ = decode_batch(ctx, batch, layout, attempts=2, capacity=capacity, to_host=False)
    n = len(infos)
    _, desc, depth = _decoded_lists(infos, regions)
    src = [RATE_OF_CODE.get(int(inf.group0_rate), 0) for inf in infos]
    ratio = [{44100: 1, 48000: 1, 88200: 2, 96000: 2, 176400: 4, 192000: 4}.get(r, 0) for r in src]
    cross = [r in (48000, 96000, 192000) for r in src]
    for i in range(n):
        if not ratio[i]:
            raise ValueError("decode_streams_resampled: stream %d runs at %d Hz: no %d Hz output" % (i, src[i], rate))
    reports = [dict(decimate=None, resample=None) for _ in range(n)]
    # stage 1: decimate by 2 / 4 where the rate asks for it; `cur` is where each stream lies after it
    cur = [(regions.d_pcm, desc[i]) for i in range(n)]
    for D in (2, 4):
        for bits in sorted(set(depth)):
            idx = [i for i in range(n) if ratio[i] == D and depth[i] == bits]
            if not idx:
                continue
            d_mid, desc_mid, d_rep = pcm_decimate(regions.d_pcm, layout, [desc[i] for i in idx], D, bits)
            for i, dm, rep in zip(idx, desc_mid, decim_list(d_rep)):
                cur[i] = (d_mid, dm)
                reports[i]["decimate"] = rep
    # stage 2: 48 kHz to 44.1 kHz, one call per buffer and depth
    for key in sorted(set((id(cur[i][0]), depth[i]) for i in range(n) if cross[i])):
        idx = [i for i in range(n) if cross[i] and (id(cur[i][0]), depth[i]) == key]
        d_out, desc_out, d_rep = pcm_resample(cur[idx[0]][0], layout, [cur[i][1] for i in idx], key[1])
        for i, do, rep in zip(idx, desc_out, decim_list(d_rep)):
            cur[i] = (d_out, do)
            reports[i]["resample"] = rep
    pcm = []
    for buf, (off, stride, frames, ch) in cur:      # (one cut per stream: the streams lie in up to three buffers)
        pcm.append(cut_regions(buf[off:off + stride * ch].cpu().numpy(), [0], [stride], [ch], [frames], layout)[0])
    return pcm, list(infos), reports


def decode_streams_downmixed(streams, out_channels=2, flags=MIX_NORMALIZED, matrices=None, device=0, layout=PCM_PLANAR,
                             ctx=None, presentation=PRESENT_FULL):
    """Decodes complete MLP byte streams and mixes each to out_channels (1 or 2) channels on the device (Context.pcm_mix),
    clamped at its own depth: through matrices[i] where the caller passes one (a PcmMix or its dict; None: the default),
    else through the default matrix of its channel assignment (mix_matrix(speaker_mask(assignment), out_channels,
    flags)).  A stream that already has out_channels channels and no matrix of the caller's is handed out as it is, with
    a report of None.  -> (pcm, infos, reports): pcm[i] int32 [out channels, frames], reports[i] = PcmMixReport.as_dict().
    ValueError for a default matrix the kernels do not take (MIX_UNITY rows whose weights sum above 2^31) or an
    assignment without a speaker mask: judged before anything is mixed.  A stream whose region the decode could not fill
    (DVDA_ST_OVERFLOW) comes out empty with a report of zeros."""
    if layout not in (PCM_PLANAR, PCM_INTERLEAVED) or out_channels not in (1, 2):
        raise HipError("decode_streams_downmixed: EINVAL (an int32 layout, 1 or 2 channels)")
    import torch
    batch = Batch(streams, device)
    with _call_context(ctx, batch, None, 0, layout, presentation) as (ctx, capacity):
        regions, infos, _ = decode_batch(ctx, batch, layout, attempts=2, capacity=capacity, to_host=False)
        n = len(infos)
        frames, desc, depth = _decoded_lists(infos, regions)
        mats = [None] * n
        for i, inf in enumerate(infos):
            if matrices is not None and matrices[i] is not None:
                mats[i] = _mix_record(matrices[i])
            elif int(regions.channels[i]) != out_channels:
                mask = speaker_mask(int(inf.assignment))
                if bin(mask).count("1") != int(regions.channels[i]):
                    raise ValueError("decode_streams_downmixed: stream %d: assignment %d names no %d channels" %
                                     (i, inf.assignment, regions.channels[i]))
                mats[i] = _mix_record(mix_matrix(mask, out_channels, flags))
                if not mix_valid(mats[i]):
                    raise ValueError("decode_streams_downmixed: stream %d: the default matrix of assignment %d with flags %d "
                                     "has a row above 2^31" % (i, inf.assignment, flags))
        reports = [None] * n
        idx_all = [i for i in range(n) if mats[i] is not None]
        # only a stream handed out as it is is copied with all its channels; of a mixed one, the mix alone
        pcm = [None] * n
        for i in range(n):
            if mats[i] is None:
                words = region_words(regions.rows[i], regions.channels[i], layout)
                part = regions.d_pcm[regions.out_off[i]:regions.out_off[i] + words].cpu().numpy()
                pcm[i] = cut_regions(part, [0], [regions.rows[i]], [regions.channels[i]], [infos[i].pcm_frames], layout)[0]
        if idx_all:
            # the mixed regions end to end; a stream handed out as it is has none
            off, pos = [0] * n, 0
            for i in idx_all:
                off[i] = pos
                pos += frames[i] * int(mats[i].out_channels)
            d_out = torch.zeros(max(pos, 1), dtype=torch.int32, device=regions.dev)
            d_off = torch.from_numpy(np.array(off, np.int64)).to(regions.dev)
            d_stride = torch.from_numpy(np.array(frames, np.int64)).to(regions.dev)
            none = PcmMix(0, 0)
            st = torch.cuda.current_stream(regions.dev).cuda_stream
            for bits in sorted(set(depth[i] for i in idx_all)):
                # one call per depth over the whole batch: a stream of another depth, or one handed out as it is, runs
                # with a matrix of no channels and is not taken
                call = [mats[i] if mats[i] is not None and depth[i] == bits else none for i in range(n)]
                rep = ctx.pcm_mix(regions.d_pcm.data_ptr(), regions.d_out_off.data_ptr(), regions.d_stride.data_ptr(),
                                  d_out.data_ptr(), d_off.data_ptr(), d_stride.data_ptr(), call, bits, n=n, stream=st)
                for i in idx_all:
                    if depth[i] == bits:
                        reports[i] = rep[i]
            host = d_out.cpu().numpy()
            cut = cut_regions(host, [off[i] for i in idx_all], [frames[i] for i in idx_all],
                              [int(mats[i].out_channels) for i in idx_all],
                              [frames[i] if reports[i]["frames"] else 0 for i in idx_all], layout)
            for i, part in zip(idx_all, cut):
                pcm[i] = part
    return pcm, list(infos), reports


class MLPDecoder:
    """Host-side mirror of the reference's mlp.h interface (src/mlp.h:29-42):

        dvda_open_mlpdecoder(parameters)         -> MLPDecoder(g0_bps, g1_bps, g0_rate, g1_rate, assignment)
        dvda_mlpdecoder_decode_packet(d, r, s)   -> d.decode_packet(bytes, samples)
        dvda_close_mlpdecoder(d)                 -> d.close()

    `samples` plays the role of the reference's aa_int: a list with one growable list/array per
    RIFF channel; decode_packet appends the PCM frames decoded by that call to every channel
    and returns their number (0 = nothing decodable yet, the bytes stay queued)."""

    def __init__(self, group_0_bps, group_1_bps, group_0_rate, group_1_rate, channel_assignment, device=0):
        self._h = lib().dvda_hip_open_mlpdecoder(group_0_bps, group_1_bps, group_0_rate, group_1_rate,
                                                 channel_assignment, device)
        if not self._h:
            raise HipError("dvda_hip_open_mlpdecoder failed (no GPU / HIP error): there is no CPU fallback")

    def decode_packet(self, data, samples):
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8)) if not isinstance(data, np.ndarray) \
            else np.ascontiguousarray(data, np.uint8)
        planar = (ctypes.POINTER(ctypes.c_int32) * 6)()
        nch = ctypes.c_uint()
        n = lib().dvda_hip_mlpdecoder_decode_packet(self._h, buf.ctypes.data if len(buf) else None, len(buf),
                                                    planar, ctypes.byref(nch))
        if n:
            for c in range(nch.value):
                samples[c].extend(np.ctypeslib.as_array(planar[c], shape=(n,)).tolist())
        return int(n)

    @property
    def status(self):
        return int(lib().dvda_hip_mlpdecoder_status(self._h))

    @property
    def queued_bytes(self):
        return int(lib().dvda_hip_mlpdecoder_queued_bytes(self._h))

    @property
    def path(self):
        """0: decoder state on the device, a call decodes its own access units; 1: batch-tier path (dvda_hip_mlpdecoder_path)"""
        return int(lib().dvda_hip_mlpdecoder_path(self._h))

    def close(self):
        if self._h:
            lib().dvda_hip_close_mlpdecoder(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


STREAM_GROUP_MAX = 256      # DVDA_STREAM_GROUP_MAX


class MLPDecoderGroup:
    """n MLPDecoders for a host that serves many streams at once (dvda_hip_open_mlpdecoder_group): the members share
    nothing and each behaves as a lone MLPDecoder fed the same packets, but one decode_packets() call decodes every
    member's packet with one launch pair.  One device, one thread at a time."""

    def __init__(self, n, device=0):
        self._h = None
        self.n = int(n)
        if 0 <= self.n < 2 ** 32:
            self._h = lib().dvda_hip_open_mlpdecoder_group(self.n, device)
        if not self._h:
            raise HipError("dvda_hip_open_mlpdecoder_group failed (no GPU / HIP error, or n outside 1..%d): "
                           "there is no CPU fallback" % STREAM_GROUP_MAX)
        self._data = (ctypes.c_void_p * self.n)()
        self._len = (ctypes.c_size_t * self.n)()
        self._frames = (ctypes.c_uint * self.n)()
        self._planar = (ctypes.POINTER(ctypes.c_int32) * (6 * self.n))()
        self._nch = (ctypes.c_uint * self.n)()

    def decode_packets(self, pieces, samples):
        """pieces: n byte arrays (None or empty: no packet for that member this time); samples: n lists of six channel
        lists, appended to as MLPDecoder.decode_packet does -> the n returns"""
        if len(pieces) != self.n or len(samples) != self.n:
            raise ValueError("a group of %d takes %d pieces and %d sample lists" % (self.n, self.n, self.n))
        keep = []
        for i, data in enumerate(pieces):
            if data is None:
                buf = np.zeros(0, np.uint8)
            elif isinstance(data, np.ndarray):
                buf = np.ascontiguousarray(data, np.uint8)
            else:
                buf = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
            keep.append(buf)
            self._data[i] = buf.ctypes.data if len(buf) else None
            self._len[i] = len(buf)
        lib().dvda_hip_mlpdecoder_group_decode_packets(self._h, self._data, self._len, self._frames, self._planar,
                                                       self._nch)
        out = []
        for i in range(self.n):
            f = int(self._frames[i])
            if f:
                for c in range(self._nch[i]):
                    samples[i][c].extend(np.ctypeslib.as_array(self._planar[6 * i + c], shape=(f,)).tolist())
            out.append(f)
        return out

    def status(self, i):
        return int(lib().dvda_hip_mlpdecoder_group_status(self._h, i))

    def queued_bytes(self, i):
        return int(lib().dvda_hip_mlpdecoder_group_queued_bytes(self._h, i))

    def path(self, i):
        """member i's MLPDecoder.path"""
        return int(lib().dvda_hip_mlpdecoder_group_path(self._h, i))

    @property
    def steps(self):
        """launch pairs the group has run so far (dvda_hip_mlpdecoder_group_steps)"""
        return int(lib().dvda_hip_mlpdecoder_group_steps(self._h))

    def close(self):
        if self._h:
            lib().dvda_hip_close_mlpdecoder_group(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pcm_decode_sectors(sectors, bits_per_sample, channels, device=0):
    """Raw-PCM AOB sectors (bytes, multiple of 2048) -> (int32 [channels, frames], bad_sectors)
    through dvda_pcm_hip_decode_sectors.  HIP only."""
    import torch
    if not torch.cuda.is_available():
        raise HipError("no GPU visible to torch: the PCM un-swizzle path is HIP-only")
    buf = np.ascontiguousarray(np.frombuffer(bytes(sectors), np.uint8)) if not isinstance(sectors, np.ndarray) \
        else np.ascontiguousarray(sectors, np.uint8)
    assert len(buf) % 2048 == 0 and len(buf)
    n = len(buf) // 2048
    dev = torch.device("cuda", device)
    d_sec = torch.from_numpy(buf).to(dev)
    cap = n * (2048 // (2 * channels * (bits_per_sample // 8))) * 2 + 2
    cap += cap & 1
    d_pcm = torch.zeros(channels * cap, dtype=torch.int32, device=dev)
    d_work = torch.zeros(int(lib().dvda_pcm_hip_workspace_words(n)), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _check(lib().dvda_pcm_hip_decode_sectors(d_sec.data_ptr(), n, bits_per_sample, channels, d_pcm.data_ptr(),
                                             cap, d_work.data_ptr(), st), "dvda_pcm_hip_decode_sectors")
    frames, bad = ctypes.c_uint64(), ctypes.c_uint32()
    _check(lib().dvda_pcm_hip_result(d_work.data_ptr(), n, ctypes.byref(frames), ctypes.byref(bad), st),
           "dvda_pcm_hip_result")
    out = d_pcm.cpu().numpy().reshape(channels, cap)[:, :frames.value].copy()
    return out, int(bad.value)


def mlp_demux_sectors(sectors, device=0):
    """AOB sectors of an MLP track -> (MLP bytes as uint8 array, bad_sectors), on the GPU."""
    import torch
    if not torch.cuda.is_available():
        raise HipError("no GPU visible to torch: the demux path is HIP-only")
    buf = np.ascontiguousarray(sectors, np.uint8)
    assert len(buf) % 2048 == 0 and len(buf)
    n = len(buf) // 2048
    dev = torch.device("cuda", device)
    d_sec = torch.from_numpy(buf).to(dev)
    d_out = torch.zeros(len(buf) + 64, dtype=torch.uint8, device=dev)
    d_work = torch.zeros(int(lib().dvda_pcm_hip_workspace_words(n)), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _check(lib().dvda_mlp_hip_demux_sectors(d_sec.data_ptr(), n, d_out.data_ptr(), len(buf), d_work.data_ptr(), st),
           "dvda_mlp_hip_demux_sectors")
    nbytes, bad = ctypes.c_uint64(), ctypes.c_uint32()
    _check(lib().dvda_pcm_hip_result(d_work.data_ptr(), n, ctypes.byref(nbytes), ctypes.byref(bad), st), "result")
    return d_out[:nbytes.value].cpu().numpy(), int(bad.value)


def pack_wav(planar, bits_per_sample, device=0):
    """int32 [channels, frames] -> interleaved little-endian WAV payload bytes, on the GPU."""
    import torch
    if not torch.cuda.is_available():
        raise HipError("no GPU visible to torch: the WAV packing path is HIP-only")
    planar = np.ascontiguousarray(planar, np.int32)
    ch, frames = planar.shape
    dev = torch.device("cuda", device)
    d_pcm = torch.from_numpy(planar).to(dev)
    d_out = torch.zeros(frames * ch * (bits_per_sample // 8) + 4, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _check(lib().dvda_mlp_hip_pack_wav(d_pcm.data_ptr(), frames, ch, frames, bits_per_sample, d_out.data_ptr(), st),
           "dvda_mlp_hip_pack_wav")
    return d_out[:frames * ch * (bits_per_sample // 8)].cpu().numpy()
