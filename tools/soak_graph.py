#!/usr/bin/env python3
"""tools/soak_graph.py [N [SEED]] -- a pipeline that reuses its staging buffers: 16 fixed slots in one device buffer,
the same pointers, total size and stream count on every call, so that the index's launch sequence is replayed as a
hipGraph from the third call on -- with other bytes and other stream lengths in the slots every time (some empty,
some random bytes, some cut short).  Every stream the oracle decodes cleanly must come out identical.  Diagnostic."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import libdvd_audio_amd as pkg  # noqa: E402
from tests import oracle_lib  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 31
oracle = oracle_lib.Oracle()
syn, hip = pkg.synth, pkg.hipdec
rng = np.random.RandomState(seed0)
SLOTS, SLOT = 16, 96 * 1024
total = SLOTS * SLOT
host = np.zeros(total + 64, np.uint8)
batch = hip.Batch(packed=(host, np.arange(SLOTS) * SLOT, np.zeros(SLOTS)))        # (bytes and lengths rewritten per call)
tstream = torch.cuda.Stream(batch.dev)
st = tstream.cuda_stream
CAP = 16384                                     # PCM frames per slot
regions = hip.PcmRegions([CAP] * SLOTS, [6] * SLOTS)
ctx = hip.Context(0, SLOTS, 1 << 14, layout=hip.PCM_PLANAR)
two = [12, 1, 0x14, 6, 9, 3, 17, 20]
bad = cases = 0
for it in range(n):
    host[:] = 0
    lens = np.zeros(SLOTS, np.int64)
    meta = [None] * SLOTS
    for j in range(SLOTS):
        kind = int(rng.randint(0, 12))
        if kind == 0:
            continue                                                            # empty slot
        S = 1 + int(rng.randint(0, 2))
        asg = int(rng.choice(two)) if S == 2 else int(rng.randint(0, 21))
        prof = int(rng.randint(0, 2))
        feats = [syn.SF_FAST, syn.SF_ALL, syn.SF["CHAINED"], 0][int(rng.randint(0, 4))] if prof else 0
        cfg = syn.make_cfg(assignment=asg, rate_code=int(rng.randint(0, 3)), n_substreams=S, n_aus=int(rng.randint(2, 60)),
                           profile=prof, features=feats, restart_interval=int(rng.randint(1, 12)))
        try:
            b, f = syn.stream(cfg, seed0 * 100000 + it * 64 + j)
        except Exception:
            continue
        if kind == 1:
            b = rng.randint(0, 256, int(rng.randint(16, 5000))).astype(np.uint8)
        elif kind == 2:
            b = b[:int(rng.randint(8, len(b)))]
        if len(b) > SLOT:
            continue
        host[j * SLOT:j * SLOT + len(b)] = b
        lens[j] = len(b)
        meta[j] = (b, asg, f)
    with torch.cuda.stream(tstream):
        batch.d_bytes.copy_(torch.from_numpy(host), non_blocking=False)
        batch.d_len.copy_(torch.from_numpy(lens), non_blocking=False)
    tstream.synchronize()
    ctx.index_batch(batch, st)
    ctx.decode(*regions.ptrs, st)
    infos = ctx.stream_info(SLOTS, stream=st)
    out = regions.d_pcm.cpu().numpy()
    for j in range(SLOTS):
        if meta[j] is None:
            if infos[j].pcm_frames != 0:
                bad += 1
                print("EMPTY SLOT DECODED", it, j, infos[j].pcm_frames)
            continue
        b, asg, f = meta[j]
        cases += 1
        nch = int(infos[j].channels) or syn.channels(asg)
        want, r, sto = oracle.decode(b, nch, CAP)
        got_n = int(infos[j].pcm_frames)
        got = out[j * CAP * 6:j * CAP * 6 + nch * CAP].reshape(nch, CAP)[:, :got_n]
        if sto == 0 and r == 0:
            ok = got_n == 0
        elif sto == 0:
            ok = (infos[j].status & ~hip.ST_BENIGN) == 0 and got_n == r and np.array_equal(got, want[:, :r])
        else:
            ok = (infos[j].status & ~hip.ST_BENIGN) != 0 or (got_n == r and np.array_equal(got, want[:, :r]))
        if not ok:
            bad += 1
            print("MISMATCH call %d slot %d asg %d oracle st %#x r %d | hip st %#x frames %d" % (it, j, asg, sto, r, infos[j].status, got_n),
                  flush=True)
ctx.close()
print("soak_graph: %d calls, %d streams, %d mismatches" % (n, cases, bad))
