"""The chain passes' cases (csrc/mlp_chain.h: k_chain_plan, the scans, k_chain_lists, the length sort, k_chain_fused;
csrc/mlp_chain_small.h: k_chain_filter, k_chain_rematrix), one table for the CPU file (tests/test_chain_model.py: the
premises, on the oracle and on the bytes) and the GPU file (tests/test_gpu_chain_edges.py: both forms, bit for bit).

TEST INFRASTRUCTURE.  Plain Python, no GPU.  Every stream comes from synth.make_cfg(profile=1, ...) with CHAINED |
FIRRAND -- every segment behind a title's first continues the FIR history of the one before it, so the title is ONE
chain -- and, where block records matter, DISC | MIXBOOKS: DISC makes every block carry decoding parameters, at the
fixed positions split_rows (synth/mlp_synth.c) gives them.

The shapes are derived from these constants (tests/test_chain_model.py holds them to the headers' text, so a changed
constant fails there instead of moving the edges away from the table):
"""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdvd-audio_amd", "csrc")

UNIT = 8                # PCM frames of a unit: mlp_chain.h "nu = R >> 3" (k_chain_fused's set-up), mlp_chain_small.h the same
FU_T = 4                # mlp_chain.h: units a chain does per turn (per barrier)
FU_DT = 3               # mlp_chain.h: turns a unit is asked for ahead of its use
FU_RING = 12            # mlp_chain.h: FU_T * FU_DT units a filter lane has in flight
FU_RECS = 8             # mlp_chain.h: access-unit records per chain in LDS
FU_BRECS = 8            # mlp_chain.h: block records per filter lane in LDS
GROUP_CHAINS = 8        # mlp_chain.h: "cpos = blockIdx.x * 8u + cl", eight chains per two-wave workgroup
CHAIN_BUCKETS = 1024    # mlp_chain.h: length classes of the sort ...
BUCKET_FRAMES = 64      # ... of 64 PCM frames each ("cls = rows >> 6"); past the last one a chain is "long"
CHAIN_DEPTH = 8         # mlp_chain_small.h: DVDA_CHAIN_DEPTH, units a lane of k_chain_filter keeps in flight
REMAT_FRAMES = 256      # mlp_chain_small.h: PCM frames of a k_chain_rematrix block ("by * 256u")
REMAT_STEP = 4096       # mlp_hip.hip chain_passes: remat_blocks = ceil(longest deferred segment / 4096)
STAMP_TURNS = 256       # mlp_chain.h: rstamp keeps the turn a ring place was asked for in a byte

RPA = {0: 40, 1: 80, 2: 160}        # PCM frames per access unit by rate code: 5, 10, 20 units


def header_constants():
    """the same constants as the two headers and the launch code state them -> dict (a regex over their text)"""
    chain = open(os.path.join(CSRC, "mlp_chain.h")).read()
    small = open(os.path.join(CSRC, "mlp_chain_small.h")).read()
    host = open(os.path.join(CSRC, "mlp_hip.hip")).read()

    def num(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    ring = re.findall(r"constexpr int FU_RING = (\w+) \* (\w+);", chain)
    assert ring == [("FU_T", "FU_DT")], ring
    out = dict(
        FU_T=num(chain, r"constexpr int FU_T = (\d+);"),
        FU_DT=num(chain, r"constexpr int FU_DT = (\d+);"),
        FU_RECS=num(chain, r"constexpr int FU_RECS = (\d+);"),
        FU_BRECS=num(chain, r"constexpr int FU_BRECS = (\d+);"),
        GROUP_CHAINS=num(chain, r"const uint32_t cpos = blockIdx\.x \* (\d+)u \+ cl;"),
        CHAIN_BUCKETS=num(chain, r"constexpr uint32_t CHAIN_BUCKETS = (\d+);"),
        BUCKET_FRAMES=1 << num(chain, r"const uint32_t cls = rows >> (\d+);"),
        CHAIN_DEPTH=num(small, r"#define DVDA_CHAIN_DEPTH (\d+)"),
        REMAT_FRAMES=num(small, r"__launch_bounds__\((\d+)\) void k_chain_rematrix"),
        REMAT_STEP=num(host, r"ca\.remat_blocks = \(w\.max_rows \+ \d+\) / (\d+) \?"),
        STAMP_TURNS=1 << num(chain, r"\(\(unsigned long long\)\(stamp & 0xFFu\) << \((\d+)u \* b\)\)"),
    )
    out["FU_RING"] = out["FU_T"] * out["FU_DT"]
    units = set(re.findall(r"nu = R >> (\d+);", chain) + re.findall(r"const uint32_t nu = R >> (\d+);", small))
    assert len(units) == 1, units
    out["UNIT"] = 1 << int(units.pop())
    steps = set(re.findall(r"by \* (\d+)u < R", small))
    assert steps == {str(out["REMAT_FRAMES"])}, steps
    return out


# ---------------------------------------------------------------------------------------------------- the table
# The eight shapes the code itself lists and no older test reaches -- a row's `paths` says which of them it is there for:
PATHS = {
    1: "short segments: below the unit ring (dma_unit repeats the last unit), ended within FU_DT + 1 turns of the set-up",
    2: "partial turns: cnt < FU_T, a unit count that is no multiple of four",
    3: "dense block records: one record per unit, next_target's escape every time, rmax exactly full",
    4: "blocks that start inside a unit: one() of filter_unit and its twin in k_chain_filter, residues 1-7",
    5: "long segments: the 8-bit turn stamps wrap, remat_blocks > 1 and the strided `by` loop",
    6: "the access-unit record ring: recno += n_au over many segments, one-unit segments",
    7: "group make-up: 1, 7, 8, 9, 17 chains, unequal lengths in one workgroup, the long class, a dead segment",
    8: "output: direct6 and the three-int2 path misaligned, capacities that end inside a unit / a 256-frame block",
}

BASE = ("CHAINED", "FIRRAND")
DISC = BASE + ("DISC", "MIXBOOKS")

Row = collections.namedtuple("Row", "group paths asg rate S n_aus interval blocks feats seed false_sync")


def _row(group, paths, rate, n_aus, interval, seed, asg=12, S=1, blocks=2, feats=BASE, false_sync=None):
    return Row(group, tuple(paths), asg, rate, S, n_aus, interval, blocks, tuple(feats), seed, false_sync)


ROWS = collections.OrderedDict()
# ---- seg_len: segment length in units = restart interval x units per access unit
ROWS["seg5_48k"] = _row("seg_len", (1, 2, 6), 0, 26, 1, 9101)               # 5 units; 25 chained one-unit segments:
ROWS["seg10_96k"] = _row("seg_len", (1, 2, 6), 1, 26, 1, 9102)              # 10 units; more than three times round the
ROWS["seg10_48k"] = _row("seg_len", (1, 2), 0, 12, 2, 9103, S=2)            # 10 units         8-slot record ring
ROWS["seg15_48k"] = _row("seg_len", (2,), 0, 15, 3, 9104)                   # 15 units: the first length above the ring
ROWS["seg20_192k"] = _row("seg_len", (6,), 2, 25, 1, 9125)                  # 20 units = 5 turns; rec_ahead = 1
ROWS["seg35_48k"] = _row("seg_len", (1, 2), 0, 23, 7, 9106)                 # 35 units, a last segment of 2 access units
# (a title's FIRST segment opens with a raw lead-in and is the fast pass's: the long shapes as the issue states them,
#  one segment each, never reach the chain passes -- kept, exact like the others, and each run again with twice the
#  access units, whose second segment is the one the name is about)
ROWS["seg1280_192k"] = _row("seg_len", (), 2, 64, 64, 9107)
ROWS["seg1280_192k_x2"] = _row("seg_len", (5,), 2, 128, 64, 9107)           # 1 280 units, 10 240 frames: remat_blocks = 3
ROWS["seg4400f_48k"] = _row("seg_len", (), 0, 110, 110, 9108)
ROWS["seg4400f_48k_x2"] = _row("seg_len", (2, 5), 0, 220, 110, 9108)        # 4 400 frames: remat_blocks = 2, a last
#                                                                             256-frame block of 48 frames
# ---- blocks: where blocks start.  split_rows: n blocks of rows // n frames, the remainder to the last
ROWS["blk3_48k"] = _row("blocks", (4,), 0, 12, 4, 9111, blocks=3, feats=DISC)            # starts 13, 26
ROWS["blk4_48k"] = _row("blocks", (4,), 0, 12, 4, 9112, blocks=4, feats=DISC)            # 10, 20, 30
ROWS["blk5_48k"] = _row("blocks", (3,), 0, 12, 4, 9113, blocks=5, feats=DISC)            # 8-frame blocks
ROWS["blk7_96k"] = _row("blocks", (4,), 1, 12, 4, 9114, blocks=7, feats=DISC)            # 11, 22, ..., 66
ROWS["blk8_96k"] = _row("blocks", (4,), 1, 12, 4, 9115, blocks=8, feats=DISC, S=2)       # 10-frame blocks
ROWS["blk8_192k"] = _row("blocks", (4,), 2, 8, 2, 9116, blocks=8, feats=DISC)            # 20-frame blocks
ROWS["varblock_96k"] = _row("blocks", (4,), 1, 16, 4, 9117, feats=BASE + ("VARBLOCK",))
ROWS["iir_96k"] = _row("blocks", (), 1, 16, 4, 9118, feats=BASE + ("IIR",))
# ---- output: the 15-unit stream and the 8-frame-block stream, six and two channels
ROWS["out_seg15_6ch"] = ROWS["seg15_48k"]._replace(group="output", paths=(8,))
ROWS["out_seg15_2ch"] = _row("output", (8,), 0, 15, 3, 9151, asg=1)
ROWS["out_blk5_6ch"] = ROWS["blk5_48k"]._replace(group="output", paths=(8,))
ROWS["out_blk5_2ch"] = _row("output", (8,), 0, 12, 4, 9162, asg=1, blocks=5, feats=DISC)
# ---- groups: the titles of the batches.  Access units 1 .. 40, so the chains of a workgroup end in different turns;
#      one or two substreams and the assignments 12 (6 channels: direct6), 1 (2) and 0x12 (5: the general store) mixed
_T_AUS = (40, 1, 24, 7, 33, 12, 3, 19, 28, 5, 36, 9, 15, 2, 22, 31, 10)
_T_INT = (4, 1, 4, 2, 3, 1, 1, 5, 4, 2, 6, 3, 1, 1, 2, 8, 3)
for _i, (_n, _r) in enumerate(zip(_T_AUS, _T_INT)):
    ROWS["t%02d" % _i] = _row("groups", (7,), (1, 0, 1, 2, 0)[_i % 5], _n, _r, 9200 + _i, asg=(12, 1, 0x12)[_i % 3],
                              S=1 + (_i // 3) % 2)
# (t01 is a single access unit: no chained segment at all.  t02 -- six channels, 96 kHz, one substream -- gets a false
#  major sync in the ignored tail of unit 10, inside its third segment: a dead segment in the middle of its chain)
ROWS["t02"] = _row("groups", (7,), 1, 24, 4, 9202, false_sync=10)
# a chain of 412 of 416 access units at 192 kHz, 65 920 PCM frames: past the last length class
ROWS["long_s1"] = _row("groups", (5, 7), 2, 416, 4, 9231)
ROWS["long_s2"] = _row("groups", (5, 7), 2, 416, 4, 9282, S=2)

# what the GPU file observed for the IIR | CHAINED row, per segment behind the first (the names of the bits of
# test_gpu_chain_edges.SEG_BITS it carries): decoded by the chain passes, frame by frame -- not the sequential pass.
# (DVDA_ST_COLD beside them says only which fast-pass kernel looked first: the lane kernels read on to the IIR taps
#  and add it, the cooperative kernel stops at the FIR taps that make the segment CHAINED.)
IIR_SEGMENTS = ["CHAINED|GENERAL"] * 3

BATCH_SIZES = (1, 7, 8, 9, 17)
BATCHES = collections.OrderedDict(("batch%d" % n, ["t%02d" % i for i in range(n)]) for n in BATCH_SIZES)
BATCHES["batch9_long_s1"] = BATCHES["batch9"] + ["long_s1"]
BATCHES["batch9_long_s2"] = BATCHES["batch9"] + ["long_s2"]

SEG_LEN = [n for n, r in ROWS.items() if r.group == "seg_len"]
BLOCKS = [n for n, r in ROWS.items() if r.group == "blocks"]
OUTPUT = [n for n, r in ROWS.items() if r.group == "output"]
TITLES = [n for n, r in ROWS.items() if r.group == "groups"]

# output group: where a region starts (int32 words), what it is filled with, how many frames it holds
MISALIGN = (1, 2, 3)
SENTINEL = 0x5A5A5A5A
CAPACITIES = ("full", "full-1", "full-7", "full-8", "full-9", "full//2+3", "1")


def capacity(which, full):
    return {"full": full, "full-1": full - 1, "full-7": full - 7, "full-8": full - 8, "full-9": full - 9,
            "full//2+3": full // 2 + 3, "1": 1}[which]


# ---------------------------------------------------------------------------------------------------- builders
Case = collections.namedtuple("Case", "name row data frames nch rpa cfg")

_cache = {}


def case(syn, name):
    """the stream of row `name` (made once per process) -> Case"""
    if name not in _cache:
        r = ROWS[name]
        assert 1 <= r.blocks <= 8           # mlp_synth.c keeps a unit's block sizes in blk[2][8]
        feats = 0
        for f in r.feats:
            feats |= syn.SF[f]
        cfg = syn.make_cfg(assignment=r.asg, rate_code=r.rate, n_substreams=r.S, n_aus=r.n_aus, profile=1, features=feats,
                           restart_interval=r.interval, blocks_per_au=r.blocks)
        data, frames = syn.stream(cfg, r.seed)
        if r.false_sync is not None:
            from tests.index_model import inject_false_sync
            data = inject_false_sync(data, r.false_sync)
        data.setflags(write=False)
        _cache[name] = Case(name, r, data, frames, syn.channels(r.asg), RPA[r.rate], cfg)
    return _cache[name]


def segment_aus(row):
    """access units of every segment of a row's stream, by the generator's rule (a restart every `interval` units)"""
    return [min(row.interval, row.n_aus - a) for a in range(0, row.n_aus, row.interval)]


def chained_units(row):
    """units of the segments BEHIND the first: the ones the chain passes decode"""
    return [n * RPA[row.rate] // UNIT for n in segment_aus(row)[1:]]


def chain_frames(row):
    """PCM frames of the row's chain: everything behind its first segment"""
    return sum(segment_aus(row)[1:]) * RPA[row.rate]


def block_starts(row):
    """where the blocks of an access unit start, by split_rows' rule: n blocks of rows // n (n lowered while that is
    below 8), the remainder to the last"""
    rows, n = RPA[row.rate], row.blocks
    while n > 1 and rows // n < 8:
        n -= 1
    return [k * (rows // n) for k in range(n)]


def lanes_for(index):
    """seg_len and blocks rows run with every lanes_per_segment; the other groups rotate it over their cases"""
    return (0, 2, 64)[index % 3]


def oracle_pcm(oracle, c):
    """(pcm [nch, frames], frames, status) of a Case by the oracle, decoded once"""
    key = ("pcm", c.name)
    if key not in _cache:
        pcm, r, st = oracle.decode(c.data, c.nch, c.frames)
        pcm.setflags(write=False)
        _cache[key] = (pcm, r, st)
    return _cache[key]


def segment_units(c):
    """from the bytes: the access unit every segment of a Case starts at, the stream's end behind them, and every
    unit's byte offset with the stream's length behind them"""
    from tests.stream_tools import frame_offsets, major_syncs
    offs = frame_offsets(c.data)
    return [offs.index(p) for p in major_syncs(c.data)] + [len(offs)], offs + [len(c.data)]


def history_matters(oracle, c):
    """per segment of a Case (False for the first): do its bytes, decoded alone -- with a FIR history of zeros -- give
    other PCM than the whole decode has for its first access unit?  Then its first block runs FIR taps on the history
    of the segment before it: DVDA_ST_CHAINED, the chain passes' to decode.  (FIRRAND now and then opens a segment
    with order 0 in every channel: that one is the fast pass's, and the title is two chains.)"""
    key = ("matters", c.name)
    if key not in _cache:
        pcm, _, _ = oracle_pcm(oracle, c)
        at, bounds = segment_units(c)
        out = [False]
        for k in range(1, len(at) - 1):
            first, n = at[k] * c.rpa, (at[k + 1] - at[k]) * c.rpa
            alone, r_alone, _ = oracle.decode(c.data[bounds[at[k]]:bounds[at[k + 1]]], c.nch, n)
            assert r_alone == n
            out.append(bool((alone[:, :c.rpa] != pcm[:, first:first + c.rpa]).any()))
        _cache[key] = out
    return _cache[key]


def chains(oracle, c):
    """PCM frames of every chain of a Case: the runs of segments that each continue the history of the one before"""
    out, run = [], 0
    for n_au, m in zip(segment_aus(c.row), history_matters(oracle, c)):
        if m:
            run += n_au * c.rpa
        elif run:
            out.append(run)
            run = 0
    return out + ([run] if run else [])
