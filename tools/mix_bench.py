"""The channel mix on the bench's headline PCM (synthetic titles, 6 ch 24 bits, 512 access units each, decoded once into
interleaved int32), every leg between two device events, in alternating rounds:

    mix62_fm / mix62_planar  dvda_pcm_hip_mix, the default 6 -> 2 matrix, frame-major -> frame-major / planar -> planar
    mix61_fm                 ... the default 6 -> 1 matrix, frame-major
    mix66_fm                 ... the 6 -> 6 identity, frame-major
    rq_yardstick             dvda_pcm_hip_requantize with bits_in == bits_out == 24 (a pure clamp), int32 -> int32, out of
                             place, frame-major, over the same input -- from the library --parent-lib names (the parent
                             commit's build), else from this one.  It moves 8 bytes per input sample, the 6 -> 2 mix 5.33.
    rq_yardstick_planar      ... planar -> planar: what the planar 6 -> 2 leg is read against
    rs6_fm                   dvda_pcm_hip_resample of the six channels (48 -> 44.1 kHz), frame-major
    mix62_then_rs2_fm        the 6 -> 2 mix, then dvda_pcm_hip_resample of its two channels
    copy_in / copy_out       the device-to-host copies into pinned memory of the 6-channel input and the 2-channel output

8 streams' output of every mixing leg is compared with tests/mix_model.py in the same run, before anything is printed.
Prints one JSON line.

    python tools/mix_bench.py [--streams 1024] [--aus 512] [--steps 20] [--parent-lib PATH --parent-commit HASH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdvd_audio_amd as pkg  # noqa: E402
from tests import mix_model as mm  # noqa: E402
from tests import resample_model as rm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=8, help="streams whose output is compared with the model")
    ap.add_argument("--parent-lib", default=None, help="libdvda_mlp_hip.so of the parent commit: rq_yardstick runs from it")
    ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from: what the result records")
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
    total = int(rows.sum())
    samples = total * ch
    out = hd.PcmRegions(rows, [ch] * n, hd.PCM_INTERLEAVED)
    ctx = hd.Context(0, n, n * ((args.aus + 7) // 8) + 64, 0, hd.PCM_INTERLEAVED)
    ctx.index_batch(batch, st)
    ctx.decode(*out.ptrs, st)
    bad = sum(1 for inf in ctx.stream_info(stream=st) if inf.status & ~hd.ST_BENIGN)
    ctx.close()
    in_off = np.array(out.out_off, np.int64)
    assert in_off[0] == 0 and in_off[-1] + rows[-1] * ch == samples      # end to end: one run of values
    d_src = out.d_pcm[:samples].clone()
    d_planar = torch.cat([d_src[o:o + r * ch].reshape(r, ch).T.contiguous().reshape(-1)
                          for o, r in zip(out.out_off, rows.tolist())])
    del out

    def records(off, stride, fr, c):
        rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
        rec["off"], rec["stride"], rec["frames"], rec["channels"] = off, stride, fr, c
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)

    def side(och, orow=rows):
        ooff = np.concatenate([[0], np.cumsum(orow * och)[:-1]])
        return dict(och=och, rows=orow, off=ooff, desc=records(ooff, orow, orow, och),
                    out=torch.zeros(int(orow.sum()) * och + 4, dtype=torch.int32, device=dev))

    I, Pl = hd.PCM_INTERLEAVED, hd.PCM_PLANAR
    d_desc = records(in_off, rows, rows, ch)
    mask = hd.speaker_mask(12)
    mats = {"62": hd.mix_matrix(mask, 2), "61": hd.mix_matrix(mask, 1), "66": mm.identity(6)}
    d_mats = {k: hd._to_device(hd._mix_records([m] * n), dev) for k, m in mats.items()}
    sides = {"62": side(2), "61": side(1), "66": side(6)}
    work = torch.empty(max(hd.pcm_mix_workspace_words(n, total), hd.pcm_requantize_workspace_words(n, total),
                           hd.pcm_resample_workspace_words(n, total)), dtype=torch.int32, device=dev)
    d_rep = torch.zeros((n, ctypes.sizeof(hd.PcmMixReport)), dtype=torch.uint8, device=dev)
    d_rep_rs = torch.zeros((n, ctypes.sizeof(hd.DecimReport)), dtype=torch.uint8, device=dev)
    rs_rows = np.array([rm.out_frames(0, int(r)) for r in rows], np.int64)
    rs6, rs2 = side(6, rs_rows), side(2, rs_rows)
    par = hd.Requant(24, 24, hd.RQ_TRUNCATE, 0, 0)

    def mix(key, d_in, layout):
        s = sides[key]
        hd._check(L.dvda_pcm_hip_mix(d_in.data_ptr(), layout, d_desc.data_ptr(), s["out"].data_ptr(), layout,
                                     s["desc"].data_ptr(), d_mats[key].data_ptr(), n, 24, total, d_rep.data_ptr(),
                                     work.data_ptr(), work.numel(), st), "dvda_pcm_hip_mix")

    def yardstick(d_in=None, layout=None):
        s = sides["66"]
        d_in, layout = (d_src, I) if d_in is None else (d_in, layout)
        hd._check(P.dvda_pcm_hip_requantize(d_in.data_ptr(), layout, d_desc.data_ptr(), s["out"].data_ptr(), layout,
                                            s["desc"].data_ptr(), None, n, ctypes.byref(par), total, d_rep.data_ptr(),
                                            work.data_ptr(), work.numel(), st), "dvda_pcm_hip_requantize")

    def resample(d_in, desc_in, s):
        hd._check(L.dvda_pcm_hip_resample(d_in.data_ptr(), I, desc_in.data_ptr(), s["out"].data_ptr(), I, s["desc"].data_ptr(),
                                          None, n, 24, int(rs_rows.sum()), d_rep_rs.data_ptr(), work.data_ptr(), work.numel(),
                                          st), "dvda_pcm_hip_resample")

    def mix_then_rs():
        mix("62", d_src, I)
        resample(sides["62"]["out"], sides["62"]["desc"], rs2)

    h_pin = torch.empty(samples, dtype=torch.int32).pin_memory()

    def copy(src, words):
        return lambda: h_pin[:words].copy_(src[:words], non_blocking=True)

    legs = {"mix62_fm": lambda: mix("62", d_src, I), "mix62_planar": lambda: mix("62", d_planar, Pl),
            "mix61_fm": lambda: mix("61", d_src, I), "mix66_fm": lambda: mix("66", d_src, I), "rq_yardstick": yardstick,
            "rq_yardstick_planar": lambda: yardstick(d_planar, Pl),
            "rs6_fm": lambda: resample(d_src, d_desc, rs6), "mix62_then_rs2_fm": mix_then_rs,
            "copy_in": copy(d_src, samples), "copy_out": copy(sides["62"]["out"], total * 2)}

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

    # outside the timed rounds, before anything is printed: every mixing leg against the model
    picks = np.linspace(0, n - 1, min(n, args.check)).astype(int)
    checked = 0

    def source(i):
        o, r = int(in_off[i]), int(rows[i])
        return d_src[o:o + r * ch].cpu().numpy().reshape(r, ch).T

    for key, d_in, layout, what in (("62", d_src, I, "6 -> 2 frame-major"), ("62", d_planar, Pl, "6 -> 2 planar"),
                                    ("61", d_src, I, "6 -> 1"), ("66", d_src, I, "6 -> 6")):
        s = sides[key]
        s["out"].zero_()
        mix(key, d_in, layout)
        torch.cuda.synchronize()
        reports = hd.mix_list(d_rep)
        for i in picks:
            want, cl = mm.mix_np(source(i), mats[key], 24)
            oo, r, och = int(s["off"][i]), int(rows[i]), s["och"]
            got = s["out"][oo:oo + r * och].cpu().numpy()
            got = got.reshape(r, och).T if layout == I else got.reshape(och, r)
            if not np.array_equal(got, want) or reports[i] != mm.report(r, cl):
                raise SystemExit("stream %d, %s: not the model's output -- no times printed" % (i, what))
            checked += 1

    res = {"streams": n, "aus": args.aus, "frames": total, "samples_in": samples, "non_benign": bad,
           "stream_legs_checked_against_model": checked, "rq_yardstick_from": ("the parent commit %s" % args.parent_commit if args.parent_commit else
                                                                          "another build" if args.parent_lib else "this build"),
           "unit": "ms between device events"}
    moved = {"mix62_fm": 4 * (6 + 2), "mix62_planar": 4 * (6 + 2), "mix61_fm": 4 * (6 + 1), "mix66_fm": 4 * 12,
             "rq_yardstick": 4 * 12, "rq_yardstick_planar": 4 * 12, "copy_in": 4 * 6, "copy_out": 4 * 2}         # bytes per frame
    for name, v in ms.items():
        m = float(np.median(v))
        res[name] = {"median_ms": round(m, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3)}
        if name in moved:
            res[name].update(bytes_per_input_sample=round(moved[name] / 6, 2), GB_per_s=round(total * moved[name] / m / 1e6, 1))
    for name, yname in (("mix62_fm", "rq_yardstick"), ("mix62_planar", "rq_yardstick_planar")):
        y = res[yname]
        res[yname + "_spread"] = round(y["max_ms"] / y["min_ms"], 3)
        res[name + "_over_yardstick"] = round(res[name]["median_ms"] / y["median_ms"], 3)
        res[name + "_verdict"] = ("no higher" if res[name]["median_ms"] <= y["median_ms"] else
                                  "equal (inside the yardstick's spread)" if res[name]["median_ms"] <= y["max_ms"] else "higher")
    res["mix_then_resample_over_resample_of_six"] = round(res["mix62_then_rs2_fm"]["median_ms"] / res["rs6_fm"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
