"""ctypes stub over libdvd_audio_hip.so (include/dvd-audio-hip.h): the disc-level API.

Reads like a program written against the reference's public header (reference
include/dvd-audio.h:59-201): open the disc, a title set, a title, a track, a track reader, then
dvda_read() until it returns 0.  Opening a track reader is where the GPU batch runs; there is no
CPU decode path behind it.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DISC_SO = os.path.join(HERE, "libdvd_audio_hip.so")

EXPORTS = [
    "dvda_open", "dvda_close", "dvda_titleset_count",
    "dvda_open_titleset", "dvda_close_titleset", "dvda_titleset_number", "dvda_title_count",
    "dvda_open_title", "dvda_close_title", "dvda_title_number", "dvda_track_count", "dvda_title_pts_length",
    "dvda_open_track", "dvda_close_track", "dvda_track_number", "dvda_track_pts_index",
    "dvda_track_pts_length", "dvda_track_first_sector", "dvda_track_last_sector",
    "dvda_open_track_reader", "dvda_close_track_reader", "dvda_codec", "dvda_bits_per_sample",
    "dvda_sample_rate", "dvda_channel_count", "dvda_riff_wave_channel_mask", "dvda_read",
    "dvda_hip_set_device", "dvda_hip_set_wav_output", "dvda_hip_reader_status", "dvda_hip_reader_total_frames",
    "dvda_hip_reader_wav_payload", "dvda_hip_open_track_reader_on", "dvda_hip_reader_wav_only",
    "dvda_hip_reader_wav_next", "dvda_hip_reader_windowed", "dvda_hip_reader_memory", "dvda_hip_reader_failed",
    "dvda_hip_release_cached_buffers", "dvda_hip_set_presentation", "dvda_hip_open_track_reader_with",
    "dvda_hip_set_digest", "dvda_hip_reader_crc32", "dvda_hip_set_levels", "dvda_hip_reader_levels",
    "dvda_hip_set_energy", "dvda_hip_reader_energy", "dvda_hip_set_requantize", "dvda_hip_reader_requantized",
    "dvda_hip_reader_source_bits", "dvda_hip_set_decimate", "dvda_hip_reader_decimated", "dvda_hip_reader_source_rate",
    "dvda_hip_set_resample", "dvda_hip_reader_resampled",
    "dvda_hip_set_downmix", "dvda_hip_reader_downmixed", "dvda_hip_reader_source_channels",
    "dvda_hip_set_conceal", "dvda_hip_reader_concealed", "dvda_hip_open_track_reader_concealing",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        from . import _build, hipdec
        _build.build_all()
        hipdec.lib()                      # torch first, then libdvda_mlp_hip.so (one HIP runtime per process)
        L = ctypes.CDLL(DISC_SO)
        vp, u, cp = ctypes.c_void_p, ctypes.c_uint, ctypes.c_char_p
        for name in ("dvda_open",):
            getattr(L, name).restype = vp
            getattr(L, name).argtypes = [cp, cp]
        for name in ("dvda_open_titleset", "dvda_open_title", "dvda_open_track"):
            getattr(L, name).restype = vp
            getattr(L, name).argtypes = [vp, u]
        L.dvda_open_track_reader.restype = vp
        L.dvda_open_track_reader.argtypes = [vp]
        for name in ("dvda_close", "dvda_close_titleset", "dvda_close_title", "dvda_close_track",
                     "dvda_close_track_reader"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [vp]
        for name in ("dvda_titleset_count", "dvda_titleset_number", "dvda_title_count", "dvda_title_number",
                     "dvda_track_count", "dvda_title_pts_length", "dvda_track_number", "dvda_track_pts_index",
                     "dvda_track_pts_length", "dvda_track_first_sector", "dvda_track_last_sector",
                     "dvda_bits_per_sample", "dvda_sample_rate", "dvda_channel_count",
                     "dvda_riff_wave_channel_mask", "dvda_hip_reader_status"):
            getattr(L, name).restype = u
            getattr(L, name).argtypes = [vp]
        L.dvda_codec.restype = ctypes.c_int
        L.dvda_codec.argtypes = [vp]
        L.dvda_read.restype = u
        L.dvda_read.argtypes = [vp, u, ctypes.POINTER(ctypes.c_int)]
        L.dvda_hip_set_device.restype = None
        L.dvda_hip_set_device.argtypes = [ctypes.c_int]
        L.dvda_hip_set_wav_output.restype = None
        L.dvda_hip_set_wav_output.argtypes = [ctypes.c_int]
        L.dvda_hip_open_track_reader_on.restype = ctypes.c_void_p
        L.dvda_hip_open_track_reader_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.dvda_hip_open_track_reader_with.restype = ctypes.c_void_p
        L.dvda_hip_open_track_reader_with.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.dvda_hip_set_presentation.restype = None
        L.dvda_hip_set_presentation.argtypes = [ctypes.c_int]
        L.dvda_hip_reader_wav_only.restype = ctypes.c_int
        L.dvda_hip_reader_wav_only.argtypes = [ctypes.c_void_p]
        L.dvda_hip_reader_total_frames.restype = ctypes.c_ulonglong
        L.dvda_hip_reader_total_frames.argtypes = [vp]
        L.dvda_hip_reader_wav_payload.restype = ctypes.c_ulonglong
        L.dvda_hip_reader_wav_payload.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_ubyte))]
        L.dvda_hip_reader_wav_next.restype = ctypes.c_ulonglong
        L.dvda_hip_reader_wav_next.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_ubyte))]
        L.dvda_hip_reader_windowed.restype = ctypes.c_int
        L.dvda_hip_reader_windowed.argtypes = [vp]
        L.dvda_hip_reader_failed.restype = ctypes.c_int
        L.dvda_hip_reader_failed.argtypes = [vp]
        L.dvda_hip_reader_memory.restype = ctypes.c_int
        L.dvda_hip_reader_memory.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
        L.dvda_hip_set_digest.restype = None
        L.dvda_hip_set_digest.argtypes = [ctypes.c_int]
        L.dvda_hip_reader_crc32.restype = ctypes.c_int
        L.dvda_hip_reader_crc32.argtypes = [vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_ulonglong)]
        L.dvda_hip_set_levels.restype = None
        L.dvda_hip_set_levels.argtypes = [ctypes.c_int]
        L.dvda_hip_reader_levels.restype = ctypes.c_int
        L.dvda_hip_reader_levels.argtypes = [vp, ctypes.POINTER(hipdec.Levels)]
        L.dvda_hip_set_energy.restype = None
        L.dvda_hip_set_energy.argtypes = [ctypes.c_uint]
        L.dvda_hip_set_requantize.restype = None
        L.dvda_hip_set_requantize.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_ulonglong]
        L.dvda_hip_reader_source_bits.restype = ctypes.c_uint
        L.dvda_hip_reader_source_bits.argtypes = [vp]
        L.dvda_hip_reader_requantized.restype = ctypes.c_int
        L.dvda_hip_reader_requantized.argtypes = [vp, ctypes.POINTER(hipdec.RequantReport)]
        L.dvda_hip_set_decimate.restype = None
        L.dvda_hip_set_decimate.argtypes = [ctypes.c_uint]
        L.dvda_hip_reader_decimated.restype = ctypes.c_int
        L.dvda_hip_reader_decimated.argtypes = [vp, ctypes.POINTER(hipdec.DecimReport)]
        L.dvda_hip_set_resample.restype = None
        L.dvda_hip_set_resample.argtypes = [ctypes.c_uint]
        L.dvda_hip_reader_resampled.restype = ctypes.c_int
        L.dvda_hip_reader_resampled.argtypes = [vp, ctypes.POINTER(hipdec.DecimReport)]
        L.dvda_hip_set_downmix.restype = None
        L.dvda_hip_set_downmix.argtypes = [ctypes.c_uint, ctypes.c_uint]
        L.dvda_hip_reader_downmixed.restype = ctypes.c_int
        L.dvda_hip_reader_downmixed.argtypes = [vp, ctypes.POINTER(hipdec.PcmMixReport)]
        L.dvda_hip_reader_source_channels.restype = ctypes.c_uint
        L.dvda_hip_reader_source_channels.argtypes = [vp]
        L.dvda_hip_reader_source_rate.restype = ctypes.c_uint
        L.dvda_hip_reader_source_rate.argtypes = [vp]
        L.dvda_hip_reader_energy.restype = ctypes.c_int
        L.dvda_hip_reader_energy.argtypes = [vp, ctypes.POINTER(hipdec.EnergyBlock), ctypes.c_ulonglong,
                                             ctypes.POINTER(ctypes.c_ulonglong)]
        L.dvda_hip_open_track_reader_concealing.restype = ctypes.c_void_p
        L.dvda_hip_open_track_reader_concealing.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
        L.dvda_hip_set_conceal.restype = None
        L.dvda_hip_set_conceal.argtypes = [ctypes.c_int]
        L.dvda_hip_reader_concealed.restype = ctypes.c_int
        L.dvda_hip_reader_concealed.argtypes = [vp, ctypes.POINTER(hipdec.ConcealSpan), u, ctypes.POINTER(u)]
        _lib = L
    return _lib


def layout(audio_ts, titleset=1):
    """[(title, track, pts_index, pts_length, first_sector, last_sector), ...] of one title set;
    host only (no GPU needed)."""
    L = lib()
    d = L.dvda_open(audio_ts.encode(), None)
    if not d:
        raise IOError("not an AUDIO_TS directory: %s" % audio_ts)
    out = []
    try:
        ts = L.dvda_open_titleset(d, titleset)
        if not ts:
            raise IOError("title set %d not found" % titleset)
        for ti in range(1, L.dvda_title_count(ts) + 1):
            t = L.dvda_open_title(ts, ti)
            for ki in range(1, L.dvda_track_count(t) + 1):
                k = L.dvda_open_track(t, ki)
                out.append((ti, ki, L.dvda_track_pts_index(k), L.dvda_track_pts_length(k),
                            L.dvda_track_first_sector(k), L.dvda_track_last_sector(k)))
                L.dvda_close_track(k)
            L.dvda_close_title(t)
        L.dvda_close_titleset(ts)
    finally:
        L.dvda_close(d)
    return out


def read_track(audio_ts, titleset, title, track, chunk=4096, wav=False, device=0, fused=False, pieces=False,
               presentation=0, digest=False, levels=False, conceal=None, energy=0, requant=None, decimate=0,
               resample=0, downmix=0):
    """Decodes one track on the GPU.  Returns a dict: codec ("PCM"/"MLP"), bits, rate, channels,
    mask, status, and pcm = int32 [frames, channels] (interleaved, RIFF-WAVE order) read with
    dvda_read() in `chunk`-frame calls -- or, with wav=True, payload = the WAV data bytes packed
    on the GPU; fused=True (with wav=True) opens the reader as a WAV-payload-only one (dvda_hip_open_track_reader_on):
    MLP tracks are decoded straight into that payload, no int32 PCM and no packing pass.  Device and output form are
    the READER's: no process-wide switch is left behind.  pieces=True (with wav=True) takes the payload piece by piece
    (dvda_hip_reader_wav_next: a long track's windows).  A track read in windows (info["windowed"]) reports the peaks of
    what it held in info["host_peak"] / info["device_peak"]; info["frames"] is then the count at the END of the read.
    presentation=1: the 2-channel presentation of a two-substream MLP track (dvda_hip_open_track_reader_with: substream 0
    alone; info["channels"] is then k and the frames have k channels).
    digest=True: the reader digests the track on the device (dvda_hip_set_digest): info["crc32"] / info["crc32_bytes"] =
    zlib's CRC-32 of the track's WAV payload and its size (None when the bit depth has no digest), and
    info["crc32_states"] = what dvda_hip_reader_crc32 returned right after the open and at the end of the read.
    levels=True: the reader makes the level report of the track's int32 PCM on the device (dvda_hip_set_levels):
    info["levels"] = the report as hipdec.Levels.as_dict() gives it (None when the reader has none: a WAV-payload-only
    reader), and info["levels_states"] = what dvda_hip_reader_levels returned right after the open and at the end.
    energy=<block_frames>: the reader makes the energy report of the track's int32 PCM on the device, on a grid of that
    block length anchored at the track's first frame (dvda_hip_set_energy): info["energy"] = the track's blocks as
    hipdec.EnergyBlock.as_dict() gives them (None when the reader has none), and info["energy_states"] = what
    dvda_hip_reader_energy returned right after the open and at the end, info["energy_counts"] the block counts then.
    requant=(bits_out, mode, seed): the reader delivers the track at bits_out bits (dvda_hip_set_requantize: reduced on
    the device, hipdec.RQ_TRUNCATE / RQ_ROUND / RQ_TPDF with `seed`, clamped); info["bits"] is then bits_out and the PCM,
    the payload and every report are of what the reader hands out.  info["requant"] = what the reduction counted as
    hipdec.RequantReport.as_dict() gives it (None when the reader does not reduce: a track below bits_out), and
    info["requant_states"] = what dvda_hip_reader_requantized returned right after the open and at the end.
    decimate=2 or 4: the reader delivers the track at its rate / decimate where that is 44 100, 48 000, 88 200 or 96 000 Hz
    (dvda_hip_set_decimate: filtered and decimated on the device, exact, clamped at the track's depth; whole-track
    readers only -- a track read in windows cannot be opened); info["rate"] and info["frames"] are then those of the
    decimated track, and the PCM, the payload, requant= and every report are of it.  info["decimate"] = what the pass
    counted as hipdec.DecimReport.as_dict() gives it (None when the reader does not decimate: any other rate),
    info["decimate_state"] = what dvda_hip_reader_decimated returned, info["source_rate"] = the rate on the disc.
    resample=44100: the reader delivers a 48 / 96 / 192 kHz track at 44 100 Hz (dvda_hip_set_resample: decimated by 2 / 4
    where the rate asks for it, then resampled by 147 / 160 on the device, exact, clamped at the track's depth;
    whole-track readers only, not together with decimate= or conceal=); info["rate"] and info["frames"] are then those of
    the 44.1 kHz track, and the PCM, the payload, requant= and every report are of it.  info["resample"] = what the
    48 -> 44.1 kHz pass counted as hipdec.DecimReport.as_dict() gives it (None when the reader does not resample: the
    44.1 kHz family), info["resample_state"] = what dvda_hip_reader_resampled returned, info["resample_decimate"] = the
    report of the decimation in front of it (None: there was none), info["source_rate"] = the rate on the disc.
    downmix=2, 1 or (out_channels, flags): the reader delivers a track of any other channel count mixed to that many
    channels (dvda_hip_set_downmix: the default matrix of the track's channel assignment with `flags`, hipdec.MIX_*, on
    the device, exact, clamped at the track's depth, IN FRONT of decimate=, resample=, requant= and every report;
    whole-track readers only, not together with conceal=); info["channels"] and info["mask"] are then those of the mix
    (0x3, mono 0x4).  info["downmix"] = what the pass counted as hipdec.PcmMixReport.as_dict() gives it (None when the
    reader does not mix: the track has that many channels already), info["downmix_state"] = what
    dvda_hip_reader_downmixed returned, info["source_channels"] = the channels on the disc.
    conceal=True: a damaged MLP track is concealed, not refused (dvda_hip_set_conceal): info["concealed"] = the spans as
    6-tuples (first_frame, frames, byte_off, byte_end, cause, flags) in track terms, and info["concealed_states"] = what
    dvda_hip_reader_concealed returned right after the open and at the end.  conceal=False says "off" explicitly; None
    (default): as the calling thread has it (dvda_hip_set_conceal), or DVDA_CONCEAL=1 in the environment while the thread
    has made no such call.  The option is this reader's (dvda_hip_open_track_reader_concealing): the thread's setting is
    not touched."""
    from . import hipdec
    L = lib()
    d = L.dvda_open(audio_ts.encode(), None)
    if not d:
        raise IOError("not an AUDIO_TS directory: %s" % audio_ts)
    ts = t = k = r = None
    try:
        ts = L.dvda_open_titleset(d, titleset)
        t = L.dvda_open_title(ts, title) if ts else None
        k = L.dvda_open_track(t, track) if t else None
        L.dvda_hip_set_digest(1 if digest else 0)
        L.dvda_hip_set_levels(1 if levels else 0)
        L.dvda_hip_set_energy(int(energy))
        if requant is not None:
            L.dvda_hip_set_requantize(int(requant[0]), int(requant[1]), int(requant[2]))
        L.dvda_hip_set_decimate(int(decimate))
        L.dvda_hip_set_resample(int(resample))
        mx = downmix if isinstance(downmix, (tuple, list)) else (downmix, 0)
        L.dvda_hip_set_downmix(int(mx[0]), int(mx[1]))
        try:
            r = L.dvda_hip_open_track_reader_concealing(k, device, 1 if (fused and wav) else 0, presentation,
                                                        -1 if conceal is None else int(bool(conceal))) if k else None
        finally:
            L.dvda_hip_set_digest(0)            # (read when the reader is opened: nothing is left behind)
            L.dvda_hip_set_levels(0)
            L.dvda_hip_set_energy(0)
            L.dvda_hip_set_requantize(0, 0, 0)
            L.dvda_hip_set_decimate(0)
            L.dvda_hip_set_resample(0)
            L.dvda_hip_set_downmix(0, 0)
        if not r:
            raise RuntimeError("track %d/%d/%d cannot be opened for reading" % (titleset, title, track))
        ch = L.dvda_channel_count(r)
        info = {"codec": "MLP" if L.dvda_codec(r) == 1 else "PCM", "bits": L.dvda_bits_per_sample(r),
                "rate": L.dvda_sample_rate(r), "channels": ch, "mask": L.dvda_riff_wave_channel_mask(r),
                "status": L.dvda_hip_reader_status(r), "frames": int(L.dvda_hip_reader_total_frames(r)),
                "wav_only": bool(L.dvda_hip_reader_wav_only(r))}
        info["windowed"] = bool(L.dvda_hip_reader_windowed(r))
        crc, nbytes = ctypes.c_uint(), ctypes.c_ulonglong()
        first_state = L.dvda_hip_reader_crc32(r, ctypes.byref(crc), ctypes.byref(nbytes)) if digest else None
        report = hipdec.Levels()
        first_levels = L.dvda_hip_reader_levels(r, ctypes.byref(report)) if levels else None
        n_blocks = ctypes.c_ulonglong()
        first_energy = L.dvda_hip_reader_energy(r, None, 0, ctypes.byref(n_blocks)) if energy else None
        first_blocks = int(n_blocks.value)
        rq_report = hipdec.RequantReport()
        first_rq = L.dvda_hip_reader_requantized(r, ctypes.byref(rq_report)) if requant is not None else None
        n_spans = ctypes.c_uint()
        first_spans = L.dvda_hip_reader_concealed(r, None, 0, ctypes.byref(n_spans)) if conceal else None
        if wav and pieces:
            got, sizes = [], []
            while True:
                p = ctypes.POINTER(ctypes.c_ubyte)()
                n = L.dvda_hip_reader_wav_next(r, ctypes.byref(p))
                if n == 0:
                    break
                got.append(bytes(ctypes.string_at(p, n)))
                sizes.append(int(n))
            info["payload"] = b"".join(got)
            info["piece_sizes"] = sizes
        elif wav:
            p = ctypes.POINTER(ctypes.c_ubyte)()
            n = L.dvda_hip_reader_wav_payload(r, ctypes.byref(p))
            info["payload"] = bytes(ctypes.string_at(p, n)) if n else b""
        else:
            parts = []
            buf = (ctypes.c_int * (chunk * ch))()
            while True:
                n = L.dvda_read(r, chunk, buf)
                if n == 0:
                    break
                parts.append(np.frombuffer(buf, dtype=np.int32, count=n * ch).reshape(n, ch).copy())
            info["pcm"] = np.concatenate(parts) if parts else np.zeros((0, ch), np.int32)
        if info["windowed"]:
            hp, dp = ctypes.c_ulonglong(), ctypes.c_ulonglong()
            L.dvda_hip_reader_memory(r, ctypes.byref(hp), ctypes.byref(dp))
            info.update(host_peak=int(hp.value), device_peak=int(dp.value), frames=int(L.dvda_hip_reader_total_frames(r)),
                        failed=bool(L.dvda_hip_reader_failed(r)), status=L.dvda_hip_reader_status(r))
        if digest:
            state = L.dvda_hip_reader_crc32(r, ctypes.byref(crc), ctypes.byref(nbytes))
            info["crc32_states"] = (first_state, state)
            info["crc32"] = int(crc.value) if state == 1 else None
            info["crc32_bytes"] = int(nbytes.value) if state == 1 else None
        if levels:
            state = L.dvda_hip_reader_levels(r, ctypes.byref(report))
            info["levels_states"] = (first_levels, state)
            info["levels"] = report.as_dict() if state == 1 else None
        if energy:
            state = L.dvda_hip_reader_energy(r, None, 0, ctypes.byref(n_blocks))
            info["energy_states"] = (first_energy, state)
            info["energy_counts"] = (first_blocks, int(n_blocks.value))
            info["energy"] = None
            if state == 1:
                arr = (hipdec.EnergyBlock * max(int(n_blocks.value), 1))()
                L.dvda_hip_reader_energy(r, arr, n_blocks.value, ctypes.byref(n_blocks))
                info["energy"] = [arr[j].as_dict() for j in range(int(n_blocks.value))]
        if requant is not None:
            state = L.dvda_hip_reader_requantized(r, ctypes.byref(rq_report))
            info["requant_states"] = (first_rq, state)
            info["requant"] = rq_report.as_dict() if state == 1 else None
            info["source_bits"] = int(L.dvda_hip_reader_source_bits(r))
        if decimate:
            dc_report = hipdec.DecimReport()
            state = L.dvda_hip_reader_decimated(r, ctypes.byref(dc_report))
            info["decimate_state"] = state
            info["decimate"] = dc_report.as_dict() if state == 1 else None
            info["source_rate"] = int(L.dvda_hip_reader_source_rate(r))
        if resample:
            rs_report, dc_report = hipdec.DecimReport(), hipdec.DecimReport()
            state = L.dvda_hip_reader_resampled(r, ctypes.byref(rs_report))
            info["resample_state"] = state
            info["resample"] = rs_report.as_dict() if state == 1 else None
            info["resample_decimate"] = dc_report.as_dict() if L.dvda_hip_reader_decimated(r, ctypes.byref(dc_report)) == 1 else None
            info["source_rate"] = int(L.dvda_hip_reader_source_rate(r))
        if mx[0]:
            mx_report = hipdec.PcmMixReport()
            state = L.dvda_hip_reader_downmixed(r, ctypes.byref(mx_report))
            info["downmix_state"] = state
            info["downmix"] = mx_report.as_dict() if state == 1 else None
            info["source_channels"] = int(L.dvda_hip_reader_source_channels(r))
        if conceal:
            state = L.dvda_hip_reader_concealed(r, None, 0, ctypes.byref(n_spans))
            arr = (hipdec.ConcealSpan * max(int(n_spans.value), 1))()
            if state >= 0:
                state = L.dvda_hip_reader_concealed(r, arr, int(n_spans.value), ctypes.byref(n_spans))
            info["concealed_states"] = (first_spans, state)
            info["concealed"] = [arr[i].as_tuple() for i in range(int(n_spans.value))] if state >= 0 else None
        return info
    finally:
        if r:
            L.dvda_close_track_reader(r)
        if k:
            L.dvda_close_track(k)
        if t:
            L.dvda_close_title(t)
        if ts:
            L.dvda_close_titleset(ts)
        L.dvda_close(d)
