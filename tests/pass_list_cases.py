"""The seven PCM passes over the shared tile-list driver (csrc/pcm_tiles.h, csrc/pcm_report_run.h: digest, levels,
compare, energy, requantize, decimate, resample) at the places of the list their own test files never reach: one table
for the CPU file (tests/test_pass_lists_model.py: the premises, from the models and the headers' constants alone) and the
GPU file (tests/test_gpu_pass_lists.py: the device against the models, exactly).

TEST INFRASTRUCTURE.  Plain numpy, no GPU.  A case is a list of Stream: planar int32 PCM, what its descriptor says of it
("taken", or one of the ways a stream is not taken) and the absolute frame it starts at (the requantizer's noise).  A
pass is an adapter (Pass): how the streams are placed, how the flat hipdec.pcm_* wrapper is called, and what the model
under tests/*_model.py expects -- the whole output buffer with its poison, and the reports.

  A  channel_cases   ch = 1 .. 8 in one call, each stream one full tile and a ragged second one whose length is no
                     multiple of the kernel's work item
  B  long_list       4200 streams in one call: the three-launch scan, a second turn of every workgroup with other
                     per-tile state than its first, find_stream over 4200 bases, a bound that cuts the list behind the
                     first turn
  C  long_stream     one stream of THREADS + 1 tiles: the second turn of a writer's join
  D  all_clip        eight channels in which every output clips: the 16-bit count fields at a tile's maximum

The kernels' constants are read out of the headers (kernel_constants), never restated.  A model's result is computed
once per content (Pass.want caches by the array's identity), so streams that share an array cost one model run: the
long list's many-tile streams do, at different places of the list and of memory."""
import collections
import os
import re
import types
import zlib

import numpy as np

from tests import compare_model as cm
from tests import decimate_model as dm
from tests import digest_model as dgm
from tests import energy_model as em
from tests import levels_model as lm
from tests import requant_model as qm
from tests import resample_model as rm
from tests.test_gpu_levels import LAYOUTS, _layout, place
from tests.test_gpu_requant import place_wav, poisoned
from tests.test_gpu_resample import mixed_pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdvd-audio_amd", "csrc")
HEADERS = dict(digest="pcm_digest.h", levels="pcm_levels.h", compare="pcm_compare.h", energy="pcm_energy.h",
               requantize="pcm_requant.h", decimate="pcm_decim.h", resample="pcm_resample.h")
SEED = 0xDEADBEEFCAFEF00D
OTHER = {"planar": "interleaved", "interleaved": "planar"}

Stream = collections.namedtuple("Stream", "pcm kind f0")       # kind: "taken", "ch0", "ch9", "short"

_K = {}


def kernel_constants():
    """what the cases depend on, out of the headers: WAVES / THREADS (pcm_tiles.h), every pass's TILE_BLOCKS, the
    decimator's LDS_WORDS and LANE_SPAN, the resampler's PAIRS, and the DVDA_*_TILE_* / PIECE defines of the contract"""
    if _K:
        return _K

    def grab(path, pattern):
        m = re.search(pattern, open(path).read())
        assert m, (path, pattern)
        return int(m.group(1))

    tiles = os.path.join(CSRC, "pcm_tiles.h")
    _K["WAVES"] = grab(tiles, r"constexpr int WAVES = (\d+);")
    assert re.search(r"constexpr int THREADS = WAVES \* 64;", open(tiles).read())
    _K["THREADS"] = 64 * _K["WAVES"]
    for name, header in HEADERS.items():
        _K["TILE_BLOCKS", name] = grab(os.path.join(CSRC, header), r"constexpr uint32_t TILE_BLOCKS = (\d+);")
    _K["LDS_WORDS"] = grab(os.path.join(CSRC, "pcm_decim.h"), r"constexpr uint32_t LDS_WORDS = (\d+);")
    _K["LANE_SPAN"] = grab(os.path.join(CSRC, "pcm_decim.h"), r"constexpr uint32_t LANE_SPAN = (\d+);")
    _K["PAIRS"] = grab(os.path.join(CSRC, "pcm_resample.h"), r"constexpr uint32_t PAIRS = (\d+);")
    inc = os.path.join(ROOT, "include", "dvda_mlp_hip.h")
    for name in ("DVDA_CRC_TILE_BYTES", "DVDA_LVL_TILE_FRAMES", "DVDA_CMP_TILE_FRAMES", "DVDA_NRG_PIECE_FRAMES",
                 "DVDA_DCM_TILE_FRAMES", "DVDA_RSM_TILE_FRAMES"):
        _K[name] = grab(inc, r"#define\s+%s\s+(\d+)u" % name)
    return _K


def decim_chunk_out(D, ch):
    """chunk_out(D, ch) of csrc/pcm_decim.h from its two constants: the largest of 1024 / 512 / 256 output frames whose
    staged input -- per channel D c + 2 H samples, one word of padding per LANE_SPAN of them, one more -- fits LDS_WORDS"""
    k = kernel_constants()

    def chan_words(c_out):
        i = D * c_out + 2 * dm.half(D)
        return i + i // k["LANE_SPAN"] + 1

    return next(c for c in (1024, 512, 256) if ch * chan_words(c) <= k["LDS_WORDS"] or c == 256)


def decim_staged_words(D, ch):
    """LDS words the chunk of (D, ch) takes"""
    k = kernel_constants()
    i = D * decim_chunk_out(D, ch) + 2 * dm.half(D)
    return ch * (i + i // k["LANE_SPAN"] + 1)


_TABLES = {}


def resample_table(hd):
    if "r" not in _TABLES:
        _TABLES["r"] = hd.resample_taps()
    return _TABLES["r"]


def decim_taps(hd, D):
    if D not in _TABLES:
        _TABLES[D] = [int(v) for v in hd.decim_taps(D)]
    return _TABLES[D]


# --------------------------------------------------------------------------------------------------------- the passes

class Pass:
    """what the cases and the two test files ask of a pass; a subclass states its own"""
    name = None
    writes = False
    untaken = ("ch0", "ch9")            # the ways a stream of the long list is not taken
    run_channels = (1, 2, 3, 4, 5, 6, 7, 8)     # the long list's two-tile streams
    bits_out = 0
    uses_f0 = False                     # the stream's first absolute frame is part of what the model is asked

    def __init__(self):
        self._want = {}
        self.key = (self.name,)

    @property
    def grid(self):
        return kernel_constants()["TILE_BLOCKS", self.name]

    @property
    def tail_tiles(self):
        """tiles of each many-tile stream at the long list's end: with them the list reaches beyond n tiles, the least
        any bound on n streams holds"""
        return 24 if self.grid == 4096 else 64

    # -- the list's arithmetic
    def unit(self, ch):
        """input frames of one full tile of a stream of ch channels"""
        return self.tile

    def tiles(self, ch, frames):
        return -(-frames // self.tile)

    def units(self, s):
        """what a taken stream adds to the bound on the list"""
        return s.pcm.shape[1]

    def max_tiles(self, n, max_total):
        return max_total // self.tile + n

    def bound_for(self, n, tiles):
        """the max_total with which the list holds exactly `tiles` tiles"""
        assert tiles >= n
        return (tiles - n) * self.tile

    # -- the model
    def model(self, hd, s):
        raise NotImplementedError

    def want(self, hd, s):
        """(output as planar int32 or None, report) of a taken stream, computed once per content"""
        key = (id(s.pcm), s.f0 if self.uses_f0 else 0)
        if key not in self._want:
            self._want[key] = self.model(hd, s) + (s.pcm,)      # (the array is kept alive: its identity is the key)
        return self._want[key][:2]

    def zero(self):
        """the report of a stream that is not taken"""
        raise NotImplementedError

    def behind(self):
        """the report of a stream whose tiles do not all lie inside the bound"""
        return self.zero()

    # -- placing
    def stage(self, hd, streams, lay_in, lay_out=None, off_in=(0, 1, 2, 3, 3, 2, 1), off_out=(2, 0, 3, 1, 1),
              slack_in=(37, 38, 37), slack_out=(11, 12, 11, 11)):
        """the input buffer and its descriptors, the reports the model expects and -- a pass that writes -- the output
        buffer before the call (every stream's own elements poisoned), what it must hold afterwards, and its
        descriptors as the device is told them"""
        st = types.SimpleNamespace(streams=streams, n=len(streams), lay_in=lay_in, lay_out=lay_out or lay_in)
        st.flat_in, true_in = place([s.pcm for s in streams], lay_in, list(slack_in), off_mod=list(off_in))
        st.true_in = true_in
        st.desc_in = [d[:3] + ({"ch0": 0, "ch9": 9}.get(s.kind, d[3]),) for d, s in zip(true_in, streams)]
        st.taken = [s.kind == "taken" for s in streams]
        wants = [self.want(hd, s) if t else None for s, t in zip(streams, st.taken)]
        st.reports = [w[1] if w else self.zero() for w in wants]
        st.total = sum(self.units(s) for s, t in zip(streams, st.taken) if t)
        st.tile_counts = [self.tiles(*s.pcm.shape) if t else 0 for s, t in zip(streams, st.taken)]
        st.base = np.concatenate([[0], np.cumsum(st.tile_counts)]).astype(np.int64)
        if self.writes:
            outs = [w[0] if w else np.zeros((s.pcm.shape[0], self.out_frames(s.pcm.shape[1])), np.int32)
                    for w, s in zip(wants, streams)]
            flat_want, true_out = self.place_out(outs, st.lay_out, list(slack_out), list(off_out))
            st.true_out = true_out
            st.start = self.poison(flat_want, true_out, st.lay_out)
            st.expect = self.poison(flat_want, [d for d, t in zip(true_out, st.taken) if not t], st.lay_out)
            st.desc_out = [d[:2] + (d[2] - 1, d[3]) if s.kind == "short" else d for d, s in zip(true_out, streams)]
        return st

    def place_out(self, outs, lay_out, slack, off):
        return place(outs, lay_out, slack, off_mod=off)

    def poison(self, flat, desc, lay_out):
        return poisoned(flat, desc, lay_out, self.bits_out)

    def cut(self, st, max_total):
        """what a run with the bound max_total must give, from what the whole run gives: -> (index of the stream the
        bound cuts, reports, and -- a pass that writes -- the output buffer with the cut stream's own elements left
        open: (expected, mask of the words that are compared))"""
        mt = self.max_tiles(st.n, max_total)
        inside = [int(st.base[i + 1]) <= mt for i in range(st.n)]
        cut = inside.index(False)
        assert st.base[cut] < mt < st.base[cut + 1] and not any(inside[cut:])
        reports = [r if ok else self.behind() for r, ok in zip(st.reports, inside)]
        if not self.writes:
            return cut, reports, None
        outside = [d for d, ok in zip(st.true_out, inside) if not ok]
        expect = self.poison(st.expect, outside, st.lay_out)
        mask = np.ones(expect.size, bool)
        own = self.poison(np.zeros(expect.size, np.int32), [st.true_out[cut]], st.lay_out)
        mask[own != 0] = False
        return cut, reports, (expect, mask)

    # -- the device
    def call(self, hd, st, max_total=None, work=None):
        """the flat hipdec.pcm_* wrapper over st -> (the output buffer or None, the reports), on the host"""
        raise NotImplementedError

    def workspace_words(self, hd, n, total):
        raise NotImplementedError

    @staticmethod
    def up(flat):
        import torch
        return torch.from_numpy(flat).to(torch.device("cuda", 0))


class Digest(Pass):
    name = "digest"
    bits = 16
    run_channels = (1, 2, 4, 8, 1, 2, 4, 8)         # the channel counts whose frames divide a tile of payload

    def __init__(self):
        super().__init__()
        self.tile = kernel_constants()["DVDA_CRC_TILE_BYTES"]

    def unit(self, ch):
        assert self.tile % (ch * self.bits // 8) == 0
        return self.tile // (ch * self.bits // 8)

    def tiles(self, ch, frames):
        return -(-frames * ch * (self.bits // 8) // self.tile)

    def units(self, s):
        return s.pcm.size * (self.bits // 8)

    def model(self, hd, s):
        pay = dgm.wav_payload(s.pcm, self.bits)
        return None, (zlib.crc32(pay) if pay else 0, len(pay))

    def zero(self):
        return (0, 0)

    def call(self, hd, st, max_total=None, work=None):
        d = self.up(st.flat_in)
        got = hd.crc_list(*hd.pcm_crc32(d, _layout(hd, st.lay_in), self.bits, st.desc_in, max_total_bytes=max_total,
                                        work=work))
        assert np.array_equal(d.cpu().numpy(), st.flat_in)
        return None, got

    def workspace_words(self, hd, n, total):
        return hd.pcm_crc32_workspace_words(n, total)


class Levels(Pass):
    name = "levels"
    bits = 24

    def __init__(self):
        super().__init__()
        self.tile = kernel_constants()["DVDA_LVL_TILE_FRAMES"]

    def model(self, hd, s):
        return None, lm.levels(s.pcm, self.bits)

    def zero(self):
        return lm.zero()

    def call(self, hd, st, max_total=None, work=None):
        d = self.up(st.flat_in)
        got = hd.levels_list(hd.pcm_levels(d, _layout(hd, st.lay_in), self.bits, st.desc_in, max_total_frames=max_total,
                                           work=work))
        assert np.array_equal(d.cpu().numpy(), st.flat_in)
        return None, got

    def workspace_words(self, hd, n, total):
        return hd.pcm_levels_workspace_words(n, total)


class Compare(Pass):
    """side A is the case's streams; side B the same values but for one value in every 97 frames, in the other layout"""
    name = "compare"

    def __init__(self):
        super().__init__()
        self.tile = kernel_constants()["DVDA_CMP_TILE_FRAMES"]
        self._b = {}

    def side_b(self, a):
        if id(a) not in self._b:
            b = np.array(a)
            ch, frames = a.shape
            f = np.arange(frames // 2, frames, 97) if frames else np.zeros(0, np.int64)
            b[f % ch, f] ^= 0x10
            self._b[id(a)] = (b, a)
        return self._b[id(a)][0]

    def model(self, hd, s):
        return None, cm.diff(s.pcm, self.side_b(s.pcm), 0)

    def zero(self):
        return dict(cm.zero(), flags=cm.CMP_SHAPE)

    def behind(self):
        return cm.zero()

    def stage(self, hd, streams, lay_in, lay_out=None, **kw):
        st = super().stage(hd, streams, lay_in, lay_out, **kw)
        st.lay_b = OTHER[lay_in]
        st.flat_b, true_b = place([self.side_b(s.pcm) for s in streams], st.lay_b, [0, 1, 2], off_mod=[3, 1, 0, 2, 2])
        st.desc_b = [d[:3] + ({"ch0": 0, "ch9": 9}.get(s.kind, d[3]),) for d, s in zip(true_b, streams)]
        return st

    def call(self, hd, st, max_total=None, work=None):
        a, b = self.up(st.flat_in), self.up(st.flat_b)
        got = hd.diff_list(hd.pcm_compare(a, _layout(hd, st.lay_in), st.desc_in, b, _layout(hd, st.lay_b), st.desc_b, 0,
                                          max_total_frames=max_total, work=work))
        assert np.array_equal(a.cpu().numpy(), st.flat_in) and np.array_equal(b.cpu().numpy(), st.flat_b)
        return None, got

    def workspace_words(self, hd, n, total):
        return hd.pcm_compare_workspace_words(n, total)


class Energy(Pass):
    """a report is (the stream's blocks, their count).  A tile of the list is a piece of a block: with B = 64 every
    block is one"""
    name = "energy"
    tail_tiles = 2000                   # the bound on this list is above 2 n tiles: the tail reaches beyond it

    def __init__(self, B=64):
        super().__init__()
        self.B = B
        self.piece = kernel_constants()["DVDA_NRG_PIECE_FRAMES"]
        self.tile = min(B, self.piece)
        self.key = (self.name, B)

    def tiles(self, ch, frames):
        return em.pieces_of_stream(frames, self.B)

    def max_tiles(self, n, max_total):
        return max_total // self.piece + max_total // self.B + 2 * n

    def bound_for(self, n, tiles):
        return next(mt for mt in range(0, (tiles + 1) * self.B, self.B) if self.max_tiles(n, mt) >= tiles)

    def model(self, hd, s):
        blocks = em.energy_fast(s.pcm, self.B)
        return None, (blocks, len(blocks))

    def zero(self):
        return ([], 0)

    def call(self, hd, st, max_total=None, work=None):
        d = self.up(st.flat_in)
        got, counts = hd.energy_lists(*hd.pcm_energy(d, _layout(hd, st.lay_in), st.desc_in, self.B,
                                                     max_total_frames=max_total, work=work))
        assert np.array_equal(d.cpu().numpy(), st.flat_in)
        return None, list(zip(got, counts))

    def workspace_words(self, hd, n, total):
        return hd.pcm_energy_workspace_words(n, total, self.B)


class Writer(Pass):
    writes = True
    untaken = ("ch0", "ch9", "short")

    def frames_for(self, out):
        """input frames of a track of `out` output frames"""
        return out

    def out_frames(self, frames):
        return frames


class Requantize(Writer):
    """24 bits to bits_out, dithered; the output layout "wav" is the payload at bits_out"""
    name = "requantize"
    bits_in, mode = 24, qm.TPDF
    uses_f0 = True

    def __init__(self, bits_out=16):
        super().__init__()
        self.bits_out = bits_out
        self.tile = self.out_tile = kernel_constants()["DVDA_LVL_TILE_FRAMES"]
        self.key = (self.name, bits_out)

    def model(self, hd, s):
        out, cl = qm.requant_np(s.pcm, self.bits_in, self.bits_out, self.mode, SEED, s.f0)
        return out, qm.report(s.pcm.shape[1], cl)

    def zero(self):
        return qm.report(0, [0] * 8)

    def place_out(self, outs, lay_out, slack, off):
        if lay_out == "wav":
            return place_wav(outs, self.bits_out)
        return place(outs, lay_out, slack, off_mod=off)

    def call(self, hd, st, max_total=None, work=None):
        d_in, d_out = self.up(st.flat_in), self.up(st.start)
        lay_out = {16: hd.PCM_WAV16, 24: hd.PCM_WAV24}[self.bits_out] if st.lay_out == "wav" else _layout(hd, st.lay_out)
        got, d_rep = hd.pcm_requantize(d_in, _layout(hd, st.lay_in), st.desc_in, self.bits_in, self.bits_out, self.mode, SEED,
                                       frame0=[s.f0 for s in st.streams], out=d_out, layout_out=lay_out,
                                       desc_out=st.desc_out, max_total_frames=max_total, work=work)
        assert got is d_out and np.array_equal(d_in.cpu().numpy(), st.flat_in)
        return d_out.cpu().numpy(), hd.requant_list(d_rep)

    def workspace_words(self, hd, n, total):
        return hd.pcm_requantize_workspace_words(n, total)


class Decimate(Writer):
    name = "decimate"

    def __init__(self, D=2, bits=24):
        super().__init__()
        self.D, self.bits = D, bits
        self.out_tile = kernel_constants()["DVDA_DCM_TILE_FRAMES"]
        self.tile = self.out_tile
        self.key = (self.name, D, bits)

    def unit(self, ch):
        return self.D * self.out_tile

    def frames_for(self, out):
        return self.D * out

    def out_frames(self, frames):
        return dm.out_frames(0, frames, self.D)

    def tiles(self, ch, frames):
        return -(-self.out_frames(frames) // self.out_tile)

    def units(self, s):
        return self.out_frames(s.pcm.shape[1])

    def model(self, hd, s):
        out, cl = dm.decimate_np(s.pcm, decim_taps(hd, self.D), self.D, self.bits)
        return out, dm.report(s.pcm.shape[1], out.shape[1], cl)

    def zero(self):
        return dm.report(0, 0, [0] * 8)

    def call(self, hd, st, max_total=None, work=None):
        d_in, d_out = self.up(st.flat_in), self.up(st.start)
        got, _, d_rep = hd.pcm_decimate(d_in, _layout(hd, st.lay_in), st.desc_in, self.D, self.bits, out=d_out,
                                        layout_out=_layout(hd, st.lay_out), desc_out=st.desc_out,
                                        max_total_out_frames=max_total, work=work)
        assert got is d_out and np.array_equal(d_in.cpu().numpy(), st.flat_in)
        return d_out.cpu().numpy(), hd.decim_list(d_rep)

    def workspace_words(self, hd, n, total):
        return hd.pcm_decimate_workspace_words(n, total)


class Resample(Writer):
    name = "resample"

    def __init__(self, bits=24):
        super().__init__()
        self.bits = bits
        self.out_tile = kernel_constants()["DVDA_RSM_TILE_FRAMES"]
        self.tile = self.out_tile
        self.in_tile = rm.DOWN * self.out_tile // rm.UP         # input frames under a tile: 64 blocks of 160
        assert self.in_tile * rm.UP == rm.DOWN * self.out_tile
        self.key = (self.name, bits)

    def unit(self, ch):
        return self.in_tile

    def frames_for(self, out):
        f = rm.DOWN * out // rm.UP
        assert rm.out_frames(0, f) == out
        return f

    def out_frames(self, frames):
        return rm.out_frames(0, frames)

    def tiles(self, ch, frames):
        return -(-self.out_frames(frames) // self.out_tile)

    def units(self, s):
        return self.out_frames(s.pcm.shape[1])

    def slice_model(self, hd, pcm, t):
        """tile t of the track alone, as a piece with its 48 frames of context: what test_resample_model.py proves equal
        to the same frames of the whole -> (output, clipped)"""
        a = t * self.in_tile
        region, frame0, before, after = rm.cut(pcm, a, min(a + self.in_tile, pcm.shape[1]), 48, 48)
        return rm.resample_np(np.ascontiguousarray(region), resample_table(hd), self.bits, frame0, before, after)

    def model(self, hd, s):
        frames = s.pcm.shape[1]
        n_t = self.tiles(s.pcm.shape[0], frames)
        if n_t <= 3:
            out, cl = rm.resample_np(s.pcm, resample_table(hd), self.bits)
        else:                           # (the whole at once is a table gather of 768 bytes per output value)
            parts = [self.slice_model(hd, s.pcm, t) for t in range(n_t)]
            out = np.concatenate([o for o, _ in parts], axis=1)
            cl = [sum(c[k] for _, c in parts) for k in range(8)]
        assert out.shape[1] == self.out_frames(frames)
        return out, rm.report(frames, out.shape[1], cl)

    def zero(self):
        return rm.report(0, 0, [0] * 8)

    def call(self, hd, st, max_total=None, work=None):
        d_in, d_out = self.up(st.flat_in), self.up(st.start)
        got, _, d_rep = hd.pcm_resample(d_in, _layout(hd, st.lay_in), st.desc_in, self.bits, out=d_out,
                                        layout_out=_layout(hd, st.lay_out), desc_out=st.desc_out,
                                        max_total_out_frames=max_total, work=work)
        assert got is d_out and np.array_equal(d_in.cpu().numpy(), st.flat_in)
        return d_out.cpu().numpy(), hd.decim_list(d_rep)

    def workspace_words(self, hd, n, total):
        return hd.pcm_resample_workspace_words(n, total)


_PASSES = {}


def the_pass(name, *args):
    """one adapter per (pass, parameters) and process: its model results are shared by every test"""
    cls = dict(digest=Digest, levels=Levels, compare=Compare, energy=Energy, requantize=Requantize, decimate=Decimate,
               resample=Resample)[name]
    if (name,) + args not in _PASSES:
        _PASSES[(name,) + args] = cls(*args)
    return _PASSES[(name,) + args]


ALL = ("digest", "levels", "compare", "energy", "requantize", "decimate", "resample")
WRITERS = ("requantize", "decimate", "resample")


def layouts_of(p):
    """(input layout, output layout) pairs a pass takes; a pass that does not write has its input's alone"""
    return [(a, b) for a in LAYOUTS for b in LAYOUTS] if p.writes else [(a, a) for a in LAYOUTS]


# --------------------------------------------------------------------------------------------------------------- part A

RAGGED = (333, 77, 501, 130, 255, 1, 999, 1023)     # frames of the second tile, ch = 1 .. 8: odd, or 2 mod 4
RAGGED_RSM = (200, 350, 500, 155, 301, 455, 149, 1000)
_CASES = {}


def channel_cases(p):
    """ch = 1 .. 8, each stream one full tile and a ragged second tile (the energy report: one full piece and a ragged
    one, which at B = 64 is 64 full tiles and a ragged one)"""
    if ("A",) + p.key not in _CASES:
        rng = np.random.default_rng(8)
        streams = []
        for ch in range(1, 9):
            if p.name == "energy":
                frames = p.piece + RAGGED[ch - 1] % 300
            elif p.name == "resample":
                frames = p.frames_for(p.out_tile + RAGGED_RSM[ch - 1])
            else:
                frames = p.frames_for(p.out_tile + RAGGED[ch - 1])
            streams.append(Stream(mixed_pcm(rng, ch, frames), "taken", (0, 1, 2, 3, 2 ** 40 - 5, 12345, 6, 7)[ch - 1]))
        _CASES[("A",) + p.key] = streams
    return _CASES[("A",) + p.key]


# --------------------------------------------------------------------------------------------------------------- part B

N_LIST = 4200
CH_CYCLE = (1, 2, 1, 3, 1, 2, 4, 1, 5, 2, 6, 1, 7, 2, 8, 1, 3)
FIRST_RUN = 1                           # the list index of the first run of eight two-tile streams
BULK_AT, BULK_N = 9, 12                 # many-tile streams of one content: they move the second run to the grid's size
SECOND_RUN = {2048: 2010, 4096: 4010}   # list index of the second run, by TILE_BLOCKS: eight indices no rule names
TAIL_AT, TAIL_N = 4101, 6               # many-tile streams behind it: the list reaches beyond any bound on n streams
CUT_STREAM = TAIL_AT + 3


def long_list(p):
    """-> (streams, info).  N_LIST streams.  Every 37th is empty; every 50th is not taken (p.untaken in turn); a run of
    eight streams of two full tiles, p.run_channels, at list positions 0 .. 15 and the same run rotated by one at the
    positions TILE_BLOCKS .. TILE_BLOCKS + 15, so that a workgroup's second turn has another channel count than its
    first; all others 1 .. 40 frames of 1 .. 8 channels, one tile each.  info: run (the two runs' first list indices),
    bulk (tiles of the shared many-tile content), cut (the stream a bound of info.max_total cuts in its middle)"""
    if ("B",) + p.key in _CASES:
        return _CASES[("B",) + p.key]
    rng = np.random.default_rng(4200)
    g = p.grid
    second = SECOND_RUN[g]
    two = {ch: mixed_pcm(rng, ch, 2 * p.unit(ch)) for ch in sorted(set(p.run_channels))}
    run2 = p.run_channels[1:] + p.run_channels[:1]
    special = {}
    for k in range(8):
        special[FIRST_RUN + k] = Stream(two[p.run_channels[k]], "taken", k % 4)
        special[second + k] = Stream(two[run2[k]], "taken", (k + 1) % 4)

    def plain(i):
        ch, frames = CH_CYCLE[i % len(CH_CYCLE)], 1 + (11 * i) % 40
        kind = "taken"
        if i % 37 == 0:
            frames = 0
        if i % 50 == 49:
            kind = p.untaken[(i // 50) % len(p.untaken)]
            kind = "ch9" if kind == "short" and frames == 0 else kind
        return ch, frames, kind

    reserved = set(special) | set(range(BULK_AT, BULK_AT + BULK_N)) | set(range(TAIL_AT, TAIL_AT + TAIL_N))
    assert not any(i % 37 == 0 or i % 50 == 49 for i in reserved)
    ones = 0
    for i in range(second):
        if i not in reserved:
            ch, frames, kind = plain(i)
            ones += p.tiles(ch, frames) if kind == "taken" else 0
    extra = g - 16 - ones               # tiles the bulk streams must hold for the second run to start at position g
    t = -(-extra // BULK_N)
    rest = extra - (BULK_N - 1) * t
    assert 1 <= rest <= t, (extra, t, rest)
    bulk = mixed_pcm(rng, 1, t * p.unit(1))
    last = mixed_pcm(rng, 1, rest * p.unit(1))
    tail = bulk if p.tail_tiles == t else mixed_pcm(rng, 1, p.tail_tiles * p.unit(1))
    for k in range(BULK_N):
        special[BULK_AT + k] = Stream(bulk if k < BULK_N - 1 else last, "taken", 4 * k)
    for k in range(TAIL_N):
        special[TAIL_AT + k] = Stream(tail, "taken", 4 * k + 1)
    streams = []
    for i in range(N_LIST):
        if i in special:
            streams.append(special[i])
            continue
        ch, frames, kind = plain(i)
        pcm = mixed_pcm(rng, ch, frames)
        streams.append(Stream(pcm, kind, (2654435761 * i) % (1 << 41)))
    counts = [p.tiles(*s.pcm.shape) if s.kind == "taken" else 0 for s in streams]
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    info = types.SimpleNamespace(run=(FIRST_RUN, second), bulk=t, counts=counts, base=base, cut=CUT_STREAM,
                                 max_total=p.bound_for(N_LIST, int(base[CUT_STREAM]) + p.tail_tiles // 2))
    _CASES[("B",) + p.key] = (streams, info)
    return _CASES[("B",) + p.key]


# --------------------------------------------------------------------------------------------------------------- part C

LOUD = {"requantize": 100, "decimate": 60, "resample": 40}      # input frames at the rails, at the stream's very end
QUIET = 1 << 14                                                 # the bound on every other value of that stream


def long_stream(p, content):
    """one 1-channel stream of THREADS + 1 tiles -- the last one 100 output frames -- beside a short 2-channel one.
    content "mixed": values that clip in the first quarter; "tail": values below QUIET, which no pass clips, but for
    the last LOUD frames, alternately at the rails of int32: every clipped output lies in the last tile"""
    if ("C", content) + p.key not in _CASES:
        k = kernel_constants()
        rng = np.random.default_rng(257 + len(content))
        frames = p.frames_for(k["THREADS"] * p.out_tile + 100)
        if content == "mixed":
            pcm = mixed_pcm(rng, 1, frames)
        else:
            pcm = rng.integers(-QUIET, QUIET, (1, frames), dtype=np.int64)
            loud = LOUD[p.name]
            pcm[0, frames - loud:] = np.where(np.arange(loud) % 2, 2 ** 31 - 1, -2 ** 31)
            pcm = pcm.astype(np.int32)
        _CASES[("C", content) + p.key] = [Stream(pcm, "taken", 0), Stream(mixed_pcm(rng, 2, 9), "taken", 3)]
    return _CASES[("C", content) + p.key]


# --------------------------------------------------------------------------------------------------------------- part D

def all_clip(p):
    """eight channels, one full tile and one frame, the channels alternately at -2^31 and 2^31 - 1 throughout"""
    if ("D",) + p.key not in _CASES:
        frames = p.frames_for(p.out_tile + 1)
        pcm = np.stack([np.full(frames, -2 ** 31 if c % 2 == 0 else 2 ** 31 - 1, np.int64) for c in range(8)])
        _CASES[("D",) + p.key] = [Stream(pcm.astype(np.int32), "taken", 0)]
    return _CASES[("D",) + p.key]


# ---------------------------------------------------------------------------------- which adapters the two files use
LIST_ARGS = dict(digest=(), levels=(), compare=(), energy=(64,), requantize=(16,), decimate=(2, 24), resample=(24,))
CLIP_ARGS = dict(requantize=(16,), decimate=(2, 16), resample=(16,))       # part D: reduced to 16 bits


def list_pass(name):
    """the adapter of parts B and C"""
    return the_pass(name, *LIST_ARGS[name])


def clip_pass(name):
    """the adapter of part D"""
    return the_pass(name, *CLIP_ARGS[name])


def channel_passes():
    """part A: (id, adapter, (input layout, output layout)) of every parametrization"""
    out = []
    for D in dm.RATIOS:
        out += [("decimate-%d-%s-%s" % (D, a, b), the_pass("decimate", D, 24), (a, b)) for a in LAYOUTS for b in LAYOUTS]
    out += [("resample-%s-%s" % (a, b), the_pass("resample", 24), (a, b)) for a in LAYOUTS for b in LAYOUTS]
    for a in LAYOUTS:
        out += [("requantize-%s-%s" % (a, b), the_pass("requantize", 16), (a, b)) for b in LAYOUTS]
        out += [("requantize-%s-wav16" % a, the_pass("requantize", 16), (a, "wav")),
                ("requantize-%s-wav24" % a, the_pass("requantize", 24), (a, "wav"))]
    for B in (64, 4410):
        out += [("energy-%d-%s" % (B, a), the_pass("energy", B), (a, a)) for a in LAYOUTS]
    return out
