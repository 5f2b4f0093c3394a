"""The resampler on the bench's headline PCM (synthetic titles, 6 ch 24 bits, 512 access units each, decoded once into
interleaved int32) taken as 48 kHz, every leg between two device events, in alternating rounds:

    rs_fm / rs_planar  dvda_pcm_hip_resample, frame-major -> frame-major / planar -> planar, clamped to 24 bits
    dc2_then_rs        dvda_pcm_hip_decimate by 2, then dvda_pcm_hip_resample of the result (the 96 kHz recipe), same buffer
    dc2_yardstick      dvda_pcm_hip_decimate by 2, frame-major, over the same buffer -- from the library --parent-lib names
                       (the parent commit's build), else from this one
    copy_in / copy_out the device-to-host copies into pinned memory of the int32 input and of the resampled int32 output
    host_one_core      the same arithmetic on one host core: a C loop over dvda_pcm_hip_resample_value (compiled here with
                       gcc against the library), over --host-streams streams, scaled to the batch

8 streams' output of every resampling leg is compared with tests/resample_model.py (dc2_then_rs: with the composition of
the two models) in the same run, before anything is printed.  Prints one JSON line.

    python tools/resample_bench.py [--streams 1024] [--aus 512] [--steps 20] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdvd_audio_amd as pkg  # noqa: E402
from tests import decimate_model as dm  # noqa: E402
from tests import resample_model as rm  # noqa: E402

MAD_NS = 1.8        # one v_mad_i64_i32 of a wave, 1.70 - 1.95 ns at two and four waves per SIMD
SIMDS = 256 * 4     # of an MI355X

HOST_C = r"""
#include <stdint.h>
int32_t dvda_pcm_hip_resample_value(const int32_t *window, uint32_t phase, unsigned bits, int *clipped);
/* one planar channel of `frames` frames, padded with 47 zeros in front and 48 behind -> out[nm] */
uint64_t resample_channel(const int32_t *padded, uint64_t nm, unsigned bits, int32_t *out)
{
    uint64_t clipped = 0;
    for (uint64_t m = 0; m < nm; m++) {
        int cl = 0;
        out[m] = dvda_pcm_hip_resample_value(padded + (160 * m) / 147, (uint32_t)((160 * m) % 147), bits, &cl);
        clipped += (uint64_t)cl;
    }
    return clipped;
}
"""


def host_loop(lib_path):
    """the C loop, compiled against the library -> (CDLL, the directory that holds it)"""
    d = tempfile.mkdtemp(prefix="rsbench")
    src, so = os.path.join(d, "host.c"), os.path.join(d, "host.so")
    open(src, "w").write(HOST_C)
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, src, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)],
                   check=True)
    h = ctypes.CDLL(so)
    h.resample_channel.restype = ctypes.c_uint64
    h.resample_channel.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--check", type=int, default=8, help="streams whose output is compared with the model")
    ap.add_argument("--host-streams", type=int, default=2, help="streams the one-core host loop is timed on")
    ap.add_argument("--parent-lib", default=None, help="libdvda_mlp_hip.so of the parent commit: dc2_yardstick runs from it")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    L = hd.lib()
    P = L
    if args.parent_lib:
        P = ctypes.CDLL(args.parent_lib)
        P.dvda_pcm_hip_decimate.argtypes = L.dvda_pcm_hip_decimate.argtypes
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
    d_planar = torch.cat([d_src[o:o + r * ch].reshape(r, ch).T.contiguous().reshape(-1)
                          for o, r in zip(out.out_off, rows.tolist())])

    def records(off, stride, fr):
        rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
        rec["off"], rec["stride"], rec["frames"], rec["channels"] = off, stride, fr, ch
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)

    def side_of(in_rows, fn, words_fn):
        orow = np.array([fn(int(r)) for r in in_rows], np.int64)
        ooff = np.concatenate([[0], np.cumsum(orow * ch)[:-1]])
        s = dict(rows=orow, off=ooff, total=int(orow.sum()), desc=records(ooff, orow, orow),
                 out=torch.zeros(int(orow.sum()) * ch + 4, dtype=torch.int32, device=dev))
        s["work"] = torch.empty(words_fn(n, s["total"]), dtype=torch.int32, device=dev)
        return s

    d_desc = records(in_off, rows, rows)
    rs = side_of(rows, lambda r: rm.out_frames(0, r), hd.pcm_resample_workspace_words)          # 48 -> 44.1
    d2 = side_of(rows, lambda r: -(-r // 2), hd.pcm_decimate_workspace_words)                   # by 2
    rs2 = side_of(d2["rows"], lambda r: rm.out_frames(0, r), hd.pcm_resample_workspace_words)   # ... then 48 -> 44.1
    d_rep = torch.zeros((n, ctypes.sizeof(hd.DecimReport)), dtype=torch.uint8, device=dev)
    d_rep2 = torch.zeros((n, ctypes.sizeof(hd.DecimReport)), dtype=torch.uint8, device=dev)
    I, Pl = hd.PCM_INTERLEAVED, hd.PCM_PLANAR

    def resample(d_in, desc_in, layout, s, rep):
        hd._check(L.dvda_pcm_hip_resample(d_in.data_ptr(), layout, desc_in.data_ptr(), s["out"].data_ptr(), layout,
                                          s["desc"].data_ptr(), None, n, 24, s["total"], rep.data_ptr(), s["work"].data_ptr(),
                                          s["work"].numel(), st), "dvda_pcm_hip_resample")

    def decimate2(lib):
        hd._check(lib.dvda_pcm_hip_decimate(d_src.data_ptr(), I, d_desc.data_ptr(), d2["out"].data_ptr(), I,
                                            d2["desc"].data_ptr(), None, n, 2, 24, d2["total"], d_rep2.data_ptr(),
                                            d2["work"].data_ptr(), d2["work"].numel(), st), "dvda_pcm_hip_decimate")

    def both():
        decimate2(L)
        resample(d2["out"], d2["desc"], I, rs2, d_rep)

    h_pin = torch.empty(samples, dtype=torch.int32).pin_memory()

    def copy(src, words):
        return lambda: h_pin[:words].copy_(src[:words], non_blocking=True)

    legs = {"rs_fm": lambda: resample(d_src, d_desc, I, rs, d_rep), "rs_planar": lambda: resample(d_planar, d_desc, Pl, rs, d_rep),
            "dc2_then_rs": both, "dc2_yardstick": lambda: decimate2(P),
            "copy_in": copy(d_src, samples), "copy_out": copy(rs["out"], rs["total"] * ch)}

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

    # outside the timed rounds, before anything is printed: every resampling leg against the model
    picks = np.linspace(0, n - 1, min(n, args.check)).astype(int)
    table = hd.resample_taps()
    taps2 = [int(v) for v in hd.decim_taps(2)]
    checked = 0

    def source(i):
        o, r = int(in_off[i]), int(rows[i])
        return d_src[o:o + r * ch].cpu().numpy().reshape(r, ch).T

    def compare(s, layout, reports, i, want, cl, frames_in, what):
        nonlocal checked
        oo, orow = int(s["off"][i]), int(s["rows"][i])
        got = s["host"][oo:oo + orow * ch]
        got = got.reshape(orow, ch).T if layout == I else got.reshape(ch, orow)
        if not np.array_equal(got, want) or reports[i] != rm.report(frames_in, orow, cl):
            raise SystemExit("stream %d, %s: not the model's output -- no times printed" % (i, what))
        checked += 1

    for d_in, layout, what in ((d_src, I, "frame-major"), (d_planar, Pl, "planar")):
        rs["out"].zero_()
        resample(d_in, d_desc, layout, rs, d_rep)
        torch.cuda.synchronize()
        rs["host"] = rs["out"].cpu().numpy()
        reports = hd.decim_list(d_rep)
        for i in picks:
            want, cl = rm.resample_np(source(i), table, 24)
            compare(rs, layout, reports, i, want, cl, int(rows[i]), what)
    rs2["out"].zero_()
    both()
    torch.cuda.synchronize()
    rs2["host"] = rs2["out"].cpu().numpy()
    reports = hd.decim_list(d_rep)
    for i in picks:
        mid, _ = dm.decimate_np(source(i), taps2, 2, 24)
        want, cl = rm.resample_np(mid, table, 24)
        compare(rs2, I, reports, i, want, cl, mid.shape[1], "by 2 then resampled")

    # the same arithmetic on one host core
    h = host_loop(pkg._build.HIP_SO)
    host_s, host_samples = 0.0, 0
    for i in picks[:args.host_streams]:
        p = source(i)
        want, cl = rm.resample_np(p, table, 24)
        for c in range(ch):
            padded = np.ascontiguousarray(np.concatenate([np.zeros(47, np.int32), p[c], np.zeros(48 + 2, np.int32)]))
            got = np.zeros(want.shape[1], np.int32)
            t0 = time.perf_counter()
            k = h.resample_channel(padded.ctypes.data, want.shape[1], 24, got.ctypes.data)
            host_s += time.perf_counter() - t0
            host_samples += p.shape[1]
            if not np.array_equal(got, want[c]) or int(k) != cl[c]:
                raise SystemExit("the host loop is not the model's output -- no times printed")

    res = {"streams": n, "aus": args.aus, "samples": samples, "int32_bytes": samples * 4, "non_benign": bad,
           "out_samples": rs["total"] * ch, "stream_legs_checked_against_model": checked,
           "dc2_yardstick_from": args.parent_lib or "this build", "unit": "ms between device events",
           "mad_ns_per_wave_instruction": MAD_NS}
    # multiply-adds: 96 per output sample by the arithmetic, 97 as the kernel issues them (291 per 3 outputs)
    mads_in = {"rs_fm": 96 * 147 / 160, "rs_planar": 96 * 147 / 160}
    for name, v in ms.items():
        m = float(np.median(v))
        res[name] = {"median_ms": round(m, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3)}
        if name in mads_in:
            mads = samples * mads_in[name]
            issued = mads * 97 / 96
            res[name].update(bytes_per_input_sample=4 * (1 + 147 / 160),
                             GB_per_s_moved=round(samples * 4 * (1 + 147 / 160) / m / 1e6, 1),
                             Gsamples_in_per_s=round(samples / m / 1e6, 2), mads_per_input_sample=mads_in[name],
                             T_lane_mads_per_s=round(mads / m / 1e9, 2),
                             share_of_mad_issue_ceiling=round(mads / m / 1e9 / (SIMDS * 64 / MAD_NS / 1e3), 3),
                             share_counting_the_padded_taps=round(issued / m / 1e9 / (SIMDS * 64 / MAD_NS / 1e3), 3))
    nz2 = sum(1 for t in taps2 if t)
    y = res["dc2_yardstick"]
    y.update(mads_per_input_sample=nz2 / 2,
             share_of_mad_issue_ceiling=round(samples * nz2 / 2 / y["median_ms"] / 1e9 / (SIMDS * 64 / MAD_NS / 1e3), 3))
    res["copy_in"]["GB_per_s"] = round(samples * 4 / res["copy_in"]["median_ms"] / 1e6, 1)
    res["copy_out"]["GB_per_s"] = round(rs["total"] * ch * 4 / res["copy_out"]["median_ms"] / 1e6, 1)
    res["host_one_core"] = {"input_samples_timed": host_samples, "seconds": round(host_s, 4),
                            "Msamples_in_per_s": round(host_samples / host_s / 1e6, 3),
                            "ms_for_the_batch_scaled": round(host_s / host_samples * samples * 1e3, 1)}
    res["rs_fm_over_copy_in"] = round(res["rs_fm"]["median_ms"] / res["copy_in"]["median_ms"], 3)
    res["yardstick_spread"] = round(y["max_ms"] / y["min_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
