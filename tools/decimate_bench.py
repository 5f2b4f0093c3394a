"""The decimation on the bench's headline PCM (synthetic titles, 6 ch 96 kHz 24 bits, 512 access units each, decoded
once into interleaved int32), every leg between two device events, in alternating rounds:

    dc2_fm / dc4_fm    dvda_pcm_hip_decimate by 2 / by 4, frame-major -> frame-major, clamped to 24 bits
    dc2_planar         ... by 2 from a planar copy of the same PCM into planar regions
    dc2_then_wav16     ... by 2 frame-major, then dvda_pcm_hip_requantize of the result to the 16-bit WAV payload (TPDF)
    rq_in_place_trunc  dvda_pcm_hip_requantize in place, truncate, over the same buffer: a pass that moves 8 bytes per
                       sample and does no arithmetic to speak of -- from the library --parent-lib names (the parent
                       commit's build), else from this one
    copy_int32 / copy_wav16_out   the device-to-host copies into pinned memory of the int32 PCM and of a 16-bit payload at
                       the rate by-2 hands out: what the track costs to fetch before and after

8 streams' output of every decimating leg is compared with tests/decimate_model.py in the same run, before anything is
printed: times of a pass that computes something else are not printed.  Prints one JSON line.

    python tools/decimate_bench.py [--streams 1024] [--aus 512] [--steps 20] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libdvd_audio_amd as pkg  # noqa: E402
from tests import decimate_model as dm  # noqa: E402
from tests import requant_model as rm  # noqa: E402

MAD_NS = 1.8        # one v_mad_i64_i32 of a wave, 1.70 - 1.95 ns at two and four waves per SIMD
SIMDS = 256 * 4     # of an MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--check", type=int, default=8, help="streams whose output is compared with the model")
    ap.add_argument("--parent-lib", default=None, help="libdvda_mlp_hip.so of the parent commit: rq_in_place_trunc runs from it")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    L = hd.lib()
    P = L
    if args.parent_lib:
        P = ctypes.CDLL(args.parent_lib)
        P.dvda_pcm_hip_requantize.argtypes = L.dvda_pcm_hip_requantize.argtypes
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=args.aus)
    flat, offs, sizes, frames = syn.batch(cfg, 1, args.streams)
    n, ch = args.streams, 6
    batch = hd.Batch(packed=(flat, offs, sizes))
    dev, st = batch.dev, batch.current_stream
    rows = frames.astype(np.int64)
    total_frames = int(rows.sum())
    samples = total_frames * ch
    out = hd.PcmRegions(rows, [ch] * n, hd.PCM_INTERLEAVED)
    ctx = hd.Context(0, n, n * ((args.aus + 7) // 8) + 64, 0, hd.PCM_INTERLEAVED)
    ctx.index_batch(batch, st)
    ctx.decode(*out.ptrs, st)
    bad = sum(1 for inf in ctx.stream_info(stream=st) if inf.status & ~hd.ST_BENIGN)
    ctx.close()
    in_off = np.array(out.out_off, np.int64)
    assert in_off[0] == 0 and in_off[-1] + rows[-1] * ch == samples      # end to end: one run of values
    d_src = out.d_pcm[:samples].clone()
    d_scratch = d_src.clone()                                            # what the in-place yardstick works on
    d_planar = torch.cat([d_src[o:o + r * ch].reshape(r, ch).T.contiguous().reshape(-1)
                          for o, r in zip(out.out_off, rows.tolist())])

    def records(off, stride, fr):
        rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
        rec["off"], rec["stride"], rec["frames"], rec["channels"] = off, stride, fr, ch
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)

    d_desc = records(in_off, rows, rows)
    side = {}
    for D in (2, 4):
        orow = -(-rows // D)
        ooff = np.concatenate([[0], np.cumsum(orow * ch)[:-1]])
        side[D] = dict(rows=orow, off=ooff, total=int(orow.sum()), desc=records(ooff, orow, orow),
                       out=torch.zeros(int(orow.sum()) * ch + 4, dtype=torch.int32, device=dev))
        side[D]["work"] = torch.empty(hd.pcm_decimate_workspace_words(n, side[D]["total"]), dtype=torch.int32, device=dev)
    d_rep = torch.zeros((n, ctypes.sizeof(hd.DecimReport)), dtype=torch.uint8, device=dev)
    d_rq_rep = torch.zeros((n, ctypes.sizeof(hd.RequantReport)), dtype=torch.uint8, device=dev)
    d_rq_work = torch.empty(hd.pcm_requantize_workspace_words(n, total_frames), dtype=torch.int32, device=dev)
    s2 = side[2]
    d_desc_wav = records(s2["off"] // 2, s2["rows"], s2["rows"])        # 16-bit payloads end to end: byte 4 * off
    d_wav = torch.zeros(s2["total"] * ch // 2 + 4, dtype=torch.int32, device=dev)
    tpdf = hd.Requant(24, 16, hd.RQ_TPDF, 0, args.seed)
    trunc = hd.Requant(24, 24, hd.RQ_TRUNCATE, 0, 0)

    def dc(D, d_in, layout):
        s = side[D]
        hd._check(L.dvda_pcm_hip_decimate(d_in.data_ptr(), layout, d_desc.data_ptr(), s["out"].data_ptr(), layout,
                                          s["desc"].data_ptr(), None, n, D, 24, s["total"], d_rep.data_ptr(),
                                          s["work"].data_ptr(), s["work"].numel(), st), "dvda_pcm_hip_decimate")

    def to_wav16():
        hd._check(L.dvda_pcm_hip_requantize(s2["out"].data_ptr(), hd.PCM_INTERLEAVED, s2["desc"].data_ptr(), d_wav.data_ptr(),
                                            hd.PCM_WAV16, d_desc_wav.data_ptr(), None, n, ctypes.byref(tpdf), s2["total"],
                                            d_rq_rep.data_ptr(), d_rq_work.data_ptr(), d_rq_work.numel(), st),
                  "dvda_pcm_hip_requantize")

    def yardstick():
        hd._check(P.dvda_pcm_hip_requantize(d_scratch.data_ptr(), hd.PCM_INTERLEAVED, d_desc.data_ptr(), d_scratch.data_ptr(),
                                            hd.PCM_INTERLEAVED, d_desc.data_ptr(), None, n, ctypes.byref(trunc), total_frames,
                                            d_rq_rep.data_ptr(), d_rq_work.data_ptr(), d_rq_work.numel(), st),
                  "dvda_pcm_hip_requantize (yardstick)")

    h_pin = torch.empty(samples, dtype=torch.int32).pin_memory()

    def copy(words):
        return lambda: h_pin[:words].copy_(d_src[:words], non_blocking=True)

    I, Pl = hd.PCM_INTERLEAVED, hd.PCM_PLANAR

    def both():
        dc(2, d_src, I)
        to_wav16()

    legs = {"dc2_fm": lambda: dc(2, d_src, I), "dc4_fm": lambda: dc(4, d_src, I), "dc2_planar": lambda: dc(2, d_planar, Pl),
            "dc2_then_wav16": both, "rq_in_place_trunc": yardstick,
            "copy_int32": copy(samples), "copy_wav16_out": copy(s2["total"] * ch // 2)}

    def between_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {k: [] for k in legs}
    for k in range(args.warmup + args.steps):
        for name, fn in legs.items():
            t = between_events(fn)
            if k >= args.warmup:
                ms[name].append(t)

    # outside the timed rounds, before anything is printed: every decimating leg against the model
    picks = np.linspace(0, n - 1, min(n, args.check)).astype(int)
    taps = {D: [int(v) for v in hd.decim_taps(D)] for D in (2, 4)}
    checked = 0
    for D, d_in, layout in ((2, d_src, I), (4, d_src, I), (2, d_planar, Pl)):
        dc(D, d_in, layout)
        torch.cuda.synchronize()
        s = side[D]
        host = s["out"].cpu().numpy()
        reports = hd.decim_list(d_rep)
        for i in picks:
            o, r = int(in_off[i]), int(rows[i])
            p = d_src[o:o + r * ch].cpu().numpy().reshape(r, ch).T
            want, cl = dm.decimate_np(p, taps[D], D, 24)
            oo, orow = int(s["off"][i]), int(s["rows"][i])
            got = host[oo:oo + orow * ch]
            got = got.reshape(orow, ch).T if layout == I else got.reshape(ch, orow)
            if not np.array_equal(got, want) or reports[i] != dm.report(r, orow, cl):
                raise SystemExit("stream %d by %d (layout %d): not the model's output -- no times printed" % (i, D, layout))
            checked += 1
    both()
    torch.cuda.synchronize()
    host = d_wav.cpu().numpy().view(np.uint8)
    for i in picks:
        o, r = int(in_off[i]), int(rows[i])
        p = d_src[o:o + r * ch].cpu().numpy().reshape(r, ch).T
        low, _ = rm.requant_np(dm.decimate_np(p, taps[2], 2, 24)[0], 24, 16, rm.TPDF, args.seed, 0)
        oo = int(s2["off"][i])
        if host[2 * oo:2 * oo + 2 * low.size].tobytes() != dm.payload(low, 16):
            raise SystemExit("stream %d: by 2 then WAV16 is not the model's payload -- no times printed" % i)

    res = {"streams": n, "aus": args.aus, "samples": samples, "int32_bytes": samples * 4, "non_benign": bad,
           "stream_legs_checked_against_model": checked, "rq_in_place_trunc_from": args.parent_lib or "this build",
           "unit": "ms between device events", "mad_ns_per_wave_instruction": MAD_NS}
    ratio_of = {"dc2_fm": 2, "dc4_fm": 4, "dc2_planar": 2, "dc2_then_wav16": 2}
    for name, v in ms.items():
        m = float(np.median(v))
        res[name] = {"median_ms": round(m, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3)}
        if name in ratio_of:
            D = ratio_of[name]
            nz = sum(1 for t in taps[D] if t)
            mads = samples * nz / D                     # non-zero multiply-adds of the pass: nz per OUTPUT sample
            res[name].update(bytes_per_input_sample=4 * (1 + 1 / D), GB_per_s_moved=round(samples * 4 * (1 + 1 / D) / m / 1e6, 1),
                             Gsamples_in_per_s=round(samples / m / 1e6, 2), mads_per_input_sample=nz / D,
                             T_lane_mads_per_s=round(mads / m / 1e9, 2),
                             share_of_mad_issue_ceiling=round(mads / m / 1e9 / (SIMDS * 64 / MAD_NS / 1e3), 3))
    res["rq_in_place_trunc"]["GB_per_s_moved"] = round(samples * 8 / res["rq_in_place_trunc"]["median_ms"] / 1e6, 1)
    res["copy_int32"]["GB_per_s"] = round(samples * 4 / res["copy_int32"]["median_ms"] / 1e6, 1)
    res["copy_wav16_out"]["GB_per_s"] = round(s2["total"] * ch * 2 / res["copy_wav16_out"]["median_ms"] / 1e6, 1)
    res["dc2_fm_over_copy_int32"] = round(res["dc2_fm"]["median_ms"] / res["copy_int32"]["median_ms"], 3)
    res["yardstick_spread"] = round(res["rq_in_place_trunc"]["max_ms"] / res["rq_in_place_trunc"]["min_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
