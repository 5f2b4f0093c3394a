"""The word-length reduction on the bench's headline PCM (synthetic titles, 6 ch 96 kHz 24 bits, 512 access units each,
decoded once into interleaved int32), every leg between two device events, in alternating rounds:

    rq_in_place      dvda_pcm_hip_requantize 24 -> 16, TPDF, int32 -> int32 in place (the same layout and descriptors)
    rq_wav16         ... int32 -> the 16-bit WAV payload in a buffer of its own
    rq_wav16_trunc   ... the same with DVDA_RQ_TRUNCATE: no noise word, what the hash costs is the difference
    rq_planar_wav16  ... from a planar copy of the same PCM
    pack_wav16       dvda_mlp_hip_pack_wav(..., 16) over the same buffer: the yardstick, the same bytes in and out and no
                     arithmetic -- from the library --parent-lib names (the parent commit's build), else from this one
    copy_int32 / copy_wav24 / copy_wav16   the device-to-host copies into pinned memory of the int32 PCM and of payloads
                     of the two sizes: what each form of the track costs to fetch

Prints one JSON line; some streams' payloads are checked against tests/requant_model.py outside the timed rounds.

    python tools/requant_bench.py [--streams 1024] [--aus 512] [--steps 20] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libdvd_audio_amd as pkg  # noqa: E402
from tests import requant_model as rm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--aus", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--check", type=int, default=8, help="streams whose payload is compared with the model")
    ap.add_argument("--parent-lib", default=None, help="libdvda_mlp_hip.so of the parent commit: pack_wav16 runs from it")
    args = ap.parse_args()
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    L = hd.lib()
    P = L
    if args.parent_lib:
        P = ctypes.CDLL(args.parent_lib)
        P.dvda_mlp_hip_pack_wav.argtypes = L.dvda_mlp_hip_pack_wav.argtypes
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
    assert out.out_off[0] == 0 and out.out_off[-1] + rows[-1] * ch == samples    # end to end: one run of values
    d_src = out.d_pcm[:samples].clone()
    d_work_pcm = d_src.clone()                                       # what the in-place leg works on
    d_planar = torch.cat([d_src[o:o + r * ch].reshape(r, ch).T.contiguous().reshape(-1)
                          for o, r in zip(out.out_off, rows.tolist())])

    def records(off, stride):
        rec = np.zeros(n, np.dtype([("off", "<u8"), ("stride", "<u8"), ("frames", "<u8"), ("channels", "<u4"), ("r", "<u4")]))
        rec["off"], rec["stride"], rec["frames"], rec["channels"] = off, stride, rows, ch
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)

    d_desc = records(out.out_off, rows)
    wav_off = np.array(out.out_off, np.int64) // 2                   # 16-bit payloads end to end: byte 4 * off
    d_desc_wav = records(wav_off, rows)
    d_wav = torch.zeros(samples // 2 + 4, dtype=torch.int32, device=dev)
    d_pack = torch.zeros(samples // 2 + 4, dtype=torch.int32, device=dev)
    d_rep = torch.zeros((n, ctypes.sizeof(hd.RequantReport)), dtype=torch.uint8, device=dev)
    d_work = torch.empty(hd.pcm_requantize_workspace_words(n, total_frames), dtype=torch.int32, device=dev)
    tpdf = hd.Requant(24, 16, hd.RQ_TPDF, 0, args.seed)
    trunc = hd.Requant(24, 16, hd.RQ_TRUNCATE, 0, 0)

    def rq(d_in, layout_in, d_out, layout_out, desc_out, par):
        hd._check(L.dvda_pcm_hip_requantize(d_in.data_ptr(), layout_in, d_desc.data_ptr(), d_out.data_ptr(), layout_out,
                                            desc_out.data_ptr(), None, n, ctypes.byref(par), total_frames, d_rep.data_ptr(),
                                            d_work.data_ptr(), d_work.numel(), st), "dvda_pcm_hip_requantize")

    def pack():
        hd._check(P.dvda_mlp_hip_pack_wav(d_src.data_ptr(), 4, 1, samples, 16, d_pack.data_ptr(), st), "dvda_mlp_hip_pack_wav")

    h_pin = torch.empty(samples, dtype=torch.int32).pin_memory()

    def copy(words):
        return lambda: h_pin[:words].copy_(d_src[:words], non_blocking=True)

    I, Pl, W16 = hd.PCM_INTERLEAVED, hd.PCM_PLANAR, hd.PCM_WAV16
    legs = {"rq_in_place": lambda: rq(d_work_pcm, I, d_work_pcm, I, d_desc, tpdf),
            "rq_wav16": lambda: rq(d_src, I, d_wav, W16, d_desc_wav, tpdf),
            "rq_wav16_trunc": lambda: rq(d_src, I, d_wav, W16, d_desc_wav, trunc),
            "rq_planar_wav16": lambda: rq(d_planar, Pl, d_wav, W16, d_desc_wav, tpdf),
            "pack_wav16": pack,
            "copy_int32": copy(samples), "copy_wav24": copy(samples * 3 // 4), "copy_wav16": copy(samples // 2)}

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

    # outside the timed rounds: the payload against the model, the planar leg against the interleaved one
    rq(d_src, I, d_wav, W16, d_desc_wav, tpdf)
    torch.cuda.synchronize()
    ref = d_wav.clone()
    reports = hd.requant_list(d_rep)
    rq(d_planar, Pl, d_wav, W16, d_desc_wav, tpdf)
    torch.cuda.synchronize()
    assert torch.equal(ref, d_wav), "the planar input's payload differs from the interleaved one's"
    host = ref.cpu().numpy().view(np.uint8)
    checked = 0
    for i in np.linspace(0, n - 1, min(n, args.check)).astype(int):
        o, r = int(out.out_off[i]), int(rows[i])
        p = d_src[o:o + r * ch].cpu().numpy().reshape(r, ch).T
        want, cl = rm.requant_np(p, 24, 16, rm.TPDF, args.seed, 0)
        assert host[2 * o:2 * o + 2 * r * ch].tobytes() == rm.payload(want, 16), "stream %d: not the model's payload" % i
        assert reports[i] == rm.report(r, cl)
        checked += 1

    res = {"streams": n, "aus": args.aus, "samples": samples, "int32_bytes": samples * 4, "non_benign": bad,
           "streams_checked_against_model": checked, "planar_equals_interleaved": True,
           "pack_wav16_from": args.parent_lib or "this build", "unit": "ms between device events"}
    moved = {"rq_in_place": 8, "rq_wav16": 6, "rq_wav16_trunc": 6, "rq_planar_wav16": 6, "pack_wav16": 6, "copy_int32": 4,
             "copy_wav24": 3, "copy_wav16": 2}
    for name, v in ms.items():
        m = float(np.median(v))
        res[name] = {"median_ms": round(m, 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                     "GB_per_s_moved": round(samples * moved[name] / m / 1e6, 1), "Gsamples_per_s": round(samples / m / 1e6, 2)}
    res["rq_wav16_over_pack_wav16"] = round(res["rq_wav16"]["median_ms"] / res["pack_wav16"]["median_ms"], 3)
    res["pack_wav16_spread"] = round(res["pack_wav16"]["max_ms"] / res["pack_wav16"]["min_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
