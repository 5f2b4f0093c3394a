#!/usr/bin/env python3
"""tools/isa_mix.py [file.s] -- instruction mix of the k_decode row loops, priced by issue class.

At two waves per SIMD (what k_decode runs at) the VALU instructions of gfx950 fall into two issue classes,
measured by tools/valu_rate.hip and recorded in profiles/r05_valu_issue_rates.txt: about 0.9 ns and about
1.8 ns per instruction and wave.  This script compiles csrc/mlp_hip.hip to assembly the way
tools/hazard_check.py does (or reads the given .s), finds every k_decode instance's row loop -- the innermost
loop that holds the filter's v_mad_i64_i32 chain, or, for the instance that parses only, the code-book
decode's v_ffbh_u32 -- and prints per instance and per region of the loop the instruction histogram, the
split into the two classes and the class-weighted cycles.

The class table is read from the rates file (its 2-waves-per-SIMD section), not typed in: an opcode's class
is its measured time against the threshold halfway between the two clusters, a class's price is its cluster's
mean.  An opcode the file does not list is reported as "unclassified" and priced as slow.

Regions, by what a basic block of the loop contains (static counts, cold branches included):
    slot k         the block with the k-th code-book decode (v_ffbh_u32): symbol, filter, history shift
    slot masks     the small blocks between two slots: which lanes carry the next slot
    chunk request  blocks that load from global memory
    commit         blocks with the ring's byte swap (v_perm_b32)
    flush          blocks that store to global memory
    rematrix + staging   what is left behind the last slot (LDS writes of the staging tile among it)
    other          the rest: row bookkeeping, the header parser and every cold branch inside the loop

One more region is printed by itself, for every instance that does not parse only: the ROW TAIL -- noise, rematrix,
staging and the row's bookkeeping.  It is not a set of whole blocks but a path: the instructions a wave executes from
behind the last slot's block to the hand-written wait for the chunk (the first s_waitcnt vmcnt(0) that waits for nothing
else, in a block without multiply-adds: a wait the compiler places for a reloaded coefficient sits among them), every
conditional branch falling through and every unconditional one taken, so cold branches are left out and the masked
blocks the wave walks through are counted.  One kind of conditional branch is taken: a forward s_cbranch_execz that skips an inner
loop.  A row has no loop of its own; what loops there is the end of a block or a synchronous ring top-up, laid out in
line under a lane mask that is empty in all but one row of a block.  The regions above and their numbers are what they
were.

Behind the row tail come the REST of the loop -- the blocks "other" lumps together and the latch the compiler lays out
in front of the header, by sub-region (rest_regions: loop control, row gate and block bookkeeping, refill test,
bypassed LSBs, the commit's test and end, flush decision, flush offsets and addresses, the flush lane by lane, the
row tail's own blocks, cold code) -- and the TURNS: the path of a lockstep wave through one turn of the loop for a
plain row, a row that requests and commits a refill, and a row that flushes (turn_path, whose docstring has the
rules by which the static walk decides a branch), each with the part of it that lies outside the slots, the slot
masks and the row tail.  tests/test_isa_row_rest.py holds that part to profiles/isa_mix_row_rest_{before,after}.txt.

tests/test_isa_budget.py imports this module and holds every build to what profiles/isa_mix_after.txt records;
tests/test_isa_row_tail.py holds the row tail to profiles/isa_mix_row_tail_{before,after}.txt."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = os.path.join(ROOT, "profiles", "r05_valu_issue_rates.txt")
HEADLINE = "k_decode<6,false,false,true,false,false,false>"


def compile_asm(out=None):
    out = out or tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", out, os.path.join(ROOT, "libdvd-audio_amd", "csrc", "mlp_hip.hip")], check=True,
                   stderr=subprocess.DEVNULL)
    return out


def compiler_version():
    try:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    except OSError:
        return "unknown"
    hip = re.search(r"HIP version:\s*(\S+)", out)
    clang = re.search(r"clang version\s*(\S+)", out)
    return "HIP %s, clang %s" % (hip.group(1) if hip else "?", clang.group(1) if clang else "?")


class Rates:
    """The two issue classes, from the 2-waves-per-SIMD section of the rates file."""

    def __init__(self, path=RATES):
        rows, section, self.clock_ghz = {}, False, 2.4
        for line in open(path):
            m = re.match(r"device .* clock (\d+) kHz", line)
            if m:
                self.clock_ghz = int(m.group(1)) / 1e6
            if line.startswith("--"):
                section = line.startswith("-- 2 wave")
                continue
            m = re.match(r"(.+?)\s+[\d.]+ ms\s+([\d.]+) ns/instr/wave", line)
            if section and m:
                rows[m.group(1).strip()] = float(m.group(2))
        base = rows["v_add_u32 (independent)"]
        self.ns = {}
        for name, ns in rows.items():
            # "A + N v_add (per instr)": A's own time is what the group takes less N adds
            m = re.match(r"(\S+ vcc) \+ (\d) v_add \(per instr\)$", name)
            if m and m.group(2) == "1":
                self.ns[m.group(1)] = ns * 2 - base
            elif re.match(r"[vs]_\w+( imm| vgpr| literal| \(vcc\)| \(sgpr pair\)| \((in)?dependent\))?$", name):
                self.ns[name] = ns
        self.ns.pop("v_cndmask_b32", None)       # back to back on one vcc: the pathological case, not the opcode's price
        v = sorted(x for x in self.ns.values())
        gap, k = max((v[i + 1] - v[i], i) for i in range(len(v) - 1))
        self.threshold = (v[k] + v[k + 1]) / 2
        fast = [x for x in v if x < self.threshold]
        slow = [x for x in v if x >= self.threshold]
        self.fast_cycles = sum(fast) / len(fast) * self.clock_ghz
        self.slow_cycles = sum(slow) / len(slow) * self.clock_ghz

    def key(self, op, operands):
        base = re.sub(r"_(e32|e64)$", "", op)
        if base.endswith("_sdwa") or base.endswith("_dpp"):
            return "v_add_u32_sdwa" if base.endswith("_sdwa") else "v_mov_b32_dpp row_shr"
        if base.startswith("v_cmp"):
            return "v_cmp (vcc)" if operands.startswith("vcc") else "v_cmp (sgpr pair)"
        if base == "v_cndmask_b32":
            return "v_cndmask vcc" if op.endswith("_e32") else "v_cndmask (sgpr pair)"
        args = [a.strip() for a in operands.split(",")]
        if base in ("v_lshlrev_b32", "v_lshrrev_b32") and len(args) > 1:
            return base + (" vgpr" if args[1].startswith("v") else " imm")
        if base == "v_and_b32" and any(re.match(r"0x[0-9a-f]+$", a) for a in args):
            return "v_and_b32 literal"
        if base in ("v_add_u32", "v_pk_mov_b32"):
            return base + " (independent)"
        return base

    def classify(self, op, operands):
        """'fast', 'slow' or 'unclassified' (priced as slow)"""
        ns = self.ns.get(self.key(op, operands))
        if ns is None:
            return "unclassified"
        return "fast" if ns < self.threshold else "slow"

    def cycles(self, cls):
        return self.fast_cycles if cls == "fast" else self.slow_cycles


def demangle_name(sym):
    m = re.match(r"_ZN3mlp8k_decodeI((?:L[ib]\d+E)+)EEvNS_10DecodeArgsE$", sym)
    if not m:
        return sym
    vals = re.findall(r"L([ib])(\d+)E", m.group(1))
    return "k_decode<%s>" % ",".join(v if t == "i" else ("true" if v == "1" else "false") for t, v in vals)


Block = collections.namedtuple("Block", "name loop ins")        # ins: [(opcode, operands, from_inline_asm)]


def _b(op):
    """the opcode without its encoding suffix"""
    return re.sub(r"_(e32|e64)$", "", op)


def kernels(path):
    """-> [(name, info dict, [Block])] for every k_decode instance in the assembly"""
    L = open(path).read().split("\n")
    out, i = [], 0
    while i < len(L):
        m = re.match(r"(_ZN3mlp8k_decodeI\w+):", L[i])
        if not m:
            i += 1
            continue
        sym, i = m.group(1), i + 1
        blocks, parents, in_asm = [Block("entry", None, [])], {}, False
        while not L[i].startswith(".Lfunc_end"):
            t = L[i].strip()
            i += 1
            m = re.match(r"(?:\.L(BB\d+_\d+):|; %(bb\.\d+):)\s*(?:;\s*(.*))?$", t)
            if m:
                name, note = m.group(1) or m.group(2), m.group(3) or ""
                notes = [note]
                while L[i].strip().startswith(";") and not L[i].strip().startswith("; %bb"):
                    notes.append(L[i].strip().lstrip("; "))
                    i += 1
                loop = None
                for n in notes:
                    mm = re.search(r"in Loop: Header=(BB\d+_\d+)", n)
                    if mm:
                        loop = mm.group(1)
                    if "Loop Header" in n:
                        loop = name
                    mm = re.match(r"=*>?\s*Parent Loop (BB\d+_\d+)", n)
                    if mm:
                        parents.setdefault(name, []).append(mm.group(1))
                blocks.append(Block(name, loop, []))
                continue
            if "ASMSTART" in t:
                in_asm = True
            if "ASMEND" in t:
                in_asm = False
            if not t or t[0] in ".;":
                continue
            mm = re.match(r"([a-z_0-9]+)\s*(.*?)\s*(?:;.*)?$", t)
            if mm:
                blocks[-1].ins.append((mm.group(1), mm.group(2), in_asm))
        info = {}
        for t in L[i:i + 120]:                   # the "; Kernel info:" comment block behind the function
            mm = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy|LDSByteSize|TotalNumSgprs):\s*(\d+)", t.strip())
            if mm:
                info.setdefault(mm.group(1), int(mm.group(2)))
            if t.startswith("; Occupancy"):
                break
        out.append((demangle_name(sym), info, blocks, parents))
    return out


def row_loop(blocks, parents):
    """-> (header label, the row loop's blocks in layout order).

    The loop is the innermost one that holds the filter chain.  The compiler lays its hot path out in one piece --
    header, chunk request, slots, rematrix, commit, flush, the branch back -- and puts what the loop also contains but
    rarely runs (the block-header parser with its own loops, error exits) behind it.  The row loop's labels are the
    ends of that piece: from the header to the last branch back, in front of the first inner loop behind the slots."""
    def holds(b, op):
        return any(_b(o) == op for o, _, _ in b.ins)
    marks = [j for j, b in enumerate(blocks) if holds(b, "v_ffbh_u32") and holds(b, "v_lshlrev_b64") and b.loop]
    if not marks:
        return None, []
    head = collections.Counter(blocks[j].loop for j in marks).most_common(1)[0][0]
    marks = [j for j in marks if blocks[j].loop == head]
    order = {b.name: j for j, b in enumerate(blocks)}
    start = order[head]
    stop = next((j for j in range(marks[-1] + 1, len(blocks)) if blocks[j].loop != head), len(blocks))
    end = stop - 1
    for j in range(stop - 1, marks[-1], -1):
        tail = [a for o, a, _ in blocks[j].ins if o == "s_branch" or o.startswith("s_cbranch")]
        if tail and order.get(tail[-1].strip().lstrip(".L"), len(blocks)) <= start:
            end = j
            break
    return head, blocks[start:end + 1]


def regions(loop_blocks):
    """-> ordered {region name: [Block]}"""
    def holds(b, pred):
        return any(pred(_b(o)) for o, _, _ in b.ins)
    slot_at = [j for j, b in enumerate(loop_blocks) if holds(b, lambda o: o == "v_ffbh_u32") and
               holds(b, lambda o: o == "v_lshlrev_b64")]
    out = collections.OrderedDict()
    for j, b in enumerate(loop_blocks):
        if j in slot_at:
            n = sum(1 for o, _, _ in b.ins if _b(o) == "v_ffbh_u32")
            k = sum(sum(1 for o, _, _ in loop_blocks[x].ins if _b(o) == "v_ffbh_u32") for x in slot_at if x < j)
            name = "slot %d" % k if n == 1 else "slots %d-%d" % (k, k + n - 1)
        elif slot_at and slot_at[0] < j < slot_at[-1] and len(b.ins) <= 16:
            name = "slot masks"
        elif holds(b, lambda o: o == "v_perm_b32"):
            name = "commit"
        elif holds(b, lambda o: o.startswith("global_store") or o.startswith("flat_store")):
            name = "flush"
        elif holds(b, lambda o: o.startswith("global_load") or o.startswith("flat_load")):
            name = "chunk request" if not slot_at or j < slot_at[0] else "other"
        elif slot_at and j > slot_at[-1] and j <= slot_at[-1] + 4 and holds(b, lambda o: o.startswith("ds_write")):
            name = "rematrix + staging"
        else:
            name = "other"
        out.setdefault(name, []).append(b)
    return out


def row_tail_path(blocks, loop_blocks):
    """-> [Block]: the fall-through path from behind the last slot to the hand-written wait, as (partial) blocks.

    `blocks` is the whole kernel in layout order (an unconditional branch may lead to a block the compiler laid out
    behind the loop's hot piece), `loop_blocks` the row loop.  Empty when the loop has no slots or no such wait."""
    def is_slot(b):
        ops = [_b(o) for o, _, _ in b.ins]
        return "v_ffbh_u32" in ops and "v_lshlrev_b64" in ops
    slots = [b.name for b in loop_blocks if is_slot(b)]
    if not slots:
        return []
    order = {b.name: j for j, b in enumerate(blocks)}
    head = loop_blocks[0].name
    j, path, seen = order[slots[-1]] + 1, [], set()
    while j < len(blocks) and blocks[j].name not in seen:
        b = blocks[j]
        seen.add(b.name)
        part, nxt = [], j + 1
        mads = any(_b(o) == "v_mad_i64_i32" for o, _, _ in b.ins)
        for op, operands, in_asm in b.ins:
            part.append((op, operands, in_asm))
            if op == "s_waitcnt" and operands.strip() == "vmcnt(0)" and not mads:
                path.append(Block(b.name, b.loop, part))
                return path
            if op == "s_branch":
                nxt = order.get(operands.strip().lstrip(".L"), len(blocks))
                break
            if op in ("s_endpgm", "s_setpc_b64"):
                nxt = len(blocks)
                break
            if op == "s_cbranch_execz":
                t = order.get(operands.strip().lstrip(".L"), -1)
                if t > j and any(x.loop not in (head, None) for x in blocks[j + 1:t]):
                    nxt = t
                    break
        path.append(Block(b.name, b.loop, part))
        j = nxt
    return []


TURNS = ("plain", "refill", "flush")
REST_REGIONS = ("loop control", "row gate and block bookkeeping", "refill test", "bypassed LSBs", "commit test and end",
                "flush decision", "flush offsets and addresses", "flush lane by lane", "row tail's blocks", "cold")


def _has(b, pred):
    return any(pred(_b(o), a) for o, a, _ in b.ins)


def _is_slot(b):
    return _has(b, lambda o, a: o == "v_ffbh_u32") and _has(b, lambda o, a: o == "v_lshlrev_b64")


def _is_pack(b):
    """a block that only packs or unpacks registers: the save and restore round cold code laid out elsewhere"""
    ops = [_b(o) for o, _, _ in b.ins if o not in ("s_waitcnt", "s_nop")]
    return len(ops) >= 8 and all(o in ("v_and_b32", "v_lshl_or_b32", "v_bfe_i32", "v_ashrrev_i32") for o in ops)


def _is_store(o, a=""):
    return o.startswith("global_store") or o.startswith("flat_store")


def _is_load(o, a=""):
    return o.startswith("global_load") or o.startswith("flat_load")


def _wait_block(blocks, loop_blocks):
    """-> name of the block with the hand-written wait for the chunk (the end of the row tail), or None"""
    tail = row_tail_path(blocks, loop_blocks)
    return tail[-1].name if tail else None


def latch_blocks(blocks, loop_blocks):
    """-> [Block]: what the compiler laid out in front of the row loop's header for the branch back (loop control)"""
    order = {b.name: j for j, b in enumerate(blocks)}
    head, out, j = loop_blocks[0].name, [], order[loop_blocks[0].name] - 1
    while j > 0 and blocks[j].loop == head and len(blocks[j].ins) <= 6:
        out.insert(0, blocks[j])
        j -= 1
    return out


def rest_regions(blocks, loop_blocks):
    """-> ordered {sub-region: [Block]}: the blocks regions() calls "other", and the latch in front of the header, by
    where they lie in the loop's hot piece and by what they hold (static counts, as regions() gives them)."""
    reg = regions(loop_blocks)
    other = {b.name for b in reg.get("other", [])}
    head = loop_blocks[0].name
    idx = {b.name: j for j, b in enumerate(loop_blocks)}
    slots = [j for j, b in enumerate(loop_blocks) if _is_slot(b)]
    wait = _wait_block(blocks, loop_blocks)
    wait_at = idx.get(wait, len(loop_blocks))
    inner = [j for j, b in enumerate(loop_blocks) if b.loop != head and slots and j < slots[0]]
    top_end = inner[-1] if inner else -1
    gate_at = next((j for j in range(slots[0] - 1, -1, -1) if any(
        o.startswith("s_cbranch") and a.strip().lstrip(".L") == wait for o, a, _ in loop_blocks[j].ins)), -1) if slots else -1
    perm = [j for j, b in enumerate(loop_blocks) if _has(b, lambda o, a: o == "v_perm_b32") and j > wait_at]
    stores = [j for j, b in enumerate(loop_blocks) if _has(b, _is_store) and j > wait_at]
    coop = [j for j, b in enumerate(loop_blocks) if _has(b, lambda o, a: o == "ds_bpermute_b32") and j > wait_at]
    coop_end = max([j for j in stores if coop and j < coop[0] + 8] or [-1])
    out = collections.OrderedDict((r, []) for r in REST_REGIONS)
    out["loop control"] += latch_blocks(blocks, loop_blocks)
    for j, b in enumerate(loop_blocks):
        if b.name not in other:
            continue
        if b.loop != head or _is_pack(b):
            r = "cold"
        elif slots and j < slots[0]:
            if _has(b, lambda o, a: o == "v_bcnt_u32_b32"):
                r = "bypassed LSBs"
            elif top_end < j < gate_at:
                r = "refill test"
            else:
                r = "row gate and block bookkeeping"
        elif j < wait_at:
            r = "row tail's blocks"
        elif j == wait_at or (perm and j <= perm[-1] + 1):
            r = "commit test and end"
        elif _has(b, lambda o, a: o in ("ds_bpermute_b32", "v_mad_u64_u32")) and (not coop or j <= coop_end):
            r = "flush offsets and addresses"
        elif (coop and j <= coop_end + 2) or (not coop and stores and j <= stores[0]):
            r = "flush decision"
        else:
            r = "flush lane by lane"
        out[r].append(b)
    return out


def turn_path(blocks, loop_blocks, turn):
    """-> [Block]: what a lockstep wave executes in one turn of the row loop, header to the branch back, as (partial)
    blocks; `turn` is "plain" (no refill, no flush), "refill" (the wave requests and commits granules) or "flush".

    A static walk, so every branch is decided by what lies on its two sides -- the blocks reachable from one side and
    not from the other, inside the loop's hot piece:
      * a side is left out when it leads out of the hot piece (cold code laid out behind it), into an inner loop (the
        synchronous top-up), into a block that only packs registers (the save and restore round the header parser),
        to the branch back before the row is decoded, to loads or the ring's byte swap in a turn that does not
        refill, or to the flush (lane permutes, 64-bit multiplies, stores) in a turn that does not flush or has
        flushed already;
      * a branch on the execution mask otherwise goes where a mask with lanes in it goes (s_cbranch_execz falls
        through, s_cbranch_execnz is taken): the wave walks its masked blocks;
      * a scalar branch otherwise goes to the side nearer to what the turn is about -- the test that every lane
        flushes (s_cmp_eq_u64 vcc, -1), the loads and swaps of a refill, the permutes and stores of a flush -- and
        falls through when neither side is.
    Between the first slot and the hand-written wait this is the row tail's rule (row_tail_path); report() checks
    that the two agree.  SQ_INSTS_VALU per launch is the check on the whole walk (docs/history.md A.15)."""
    if not loop_blocks:
        return []
    order = {b.name: j for j, b in enumerate(blocks)}
    piece = {b.name for b in loop_blocks}
    head = loop_blocks[0].name
    h = order[head]
    latch = {b.name for b in latch_blocks(blocks, loop_blocks)}
    wait = _wait_block(blocks, loop_blocks)
    state = dict(past_wait=False, stored=False, flushed=False)

    def tgt(a):
        return a.strip().lstrip(".L")

    def edges(j, pos):
        """-> successor block indices of blocks[j] from instruction `pos` on (None: out of the hot piece or back)"""
        out = []
        for o, a, _ in blocks[j].ins[pos:]:
            if o == "s_branch" or o.startswith("s_cbranch"):
                out.append(order[tgt(a)] if tgt(a) in piece else None)
                if o == "s_branch":
                    return out
            if o in ("s_endpgm", "s_setpc_b64"):
                return out
        out.append(j + 1 if j + 1 < len(blocks) and blocks[j + 1].name in piece else None)
        return out

    def reach(starts):
        seen, todo = set(), [s for s in starts if s is not None]
        while todo:
            j = todo.pop()
            if j in seen or j == h:
                continue
            seen.add(j)
            todo += [e for e in edges(j, 0) if e is not None]
        return seen

    def unwanted(b):
        if b.loop != head or _is_pack(b):
            return True
        if turn != "refill" and (_has(b, _is_load) or _has(b, lambda o, a: o == "v_perm_b32")):
            return True
        if (turn != "flush" or state["flushed"]) and (_has(b, _is_store) or
                                                       _has(b, lambda o, a: o in ("ds_bpermute_b32", "v_mad_u64_u32"))):
            return True
        return False

    def wanted(b):
        if _has(b, lambda o, a: o == "s_cmp_eq_u64" and a.replace(" ", "") == "vcc,-1"):
            return True
        if turn == "refill" and (_has(b, _is_load) or _has(b, lambda o, a: o == "v_perm_b32")):
            return True
        return turn == "flush" and not state["flushed"] and (
            _has(b, _is_store) or _has(b, lambda o, a: o in ("ds_bpermute_b32", "v_mad_u64_u32")))

    def side(starts, direct_out, other):
        """-> (left out?, distance to what the turn is about) of the side that starts at block indices `starts`"""
        if direct_out:
            return True, None
        mine = reach(starts) - other
        if any(unwanted(blocks[j]) for j in mine):
            return True, None
        dist, front, seen = 0, [s for s in starts if s in mine], set()
        while front:
            if any(wanted(blocks[j]) for j in front):
                return False, dist
            seen |= set(front)
            front = [e for j in front for e in edges(j, 0) if e in mine and e not in seen]
            dist += 1
        return False, None

    path, j, seen = [], h, set()
    while j is not None and j not in seen:
        seen.add(j)
        b = blocks[j]
        if b.name == wait:
            state["past_wait"] = True
        part, nxt = [], (j + 1 if j + 1 < len(blocks) else None)
        for pos, (op, operands, in_asm) in enumerate(b.ins):
            part.append((op, operands, in_asm))
            if _is_store(_b(op)):
                state["stored"] = True
            if op == "s_branch":
                nxt = order.get(tgt(operands))
                break
            if op in ("s_endpgm", "s_setpc_b64"):
                nxt = None
                break
            if not op.startswith("s_cbranch"):
                continue
            t = tgt(operands)
            back = t in latch or t == head
            t_out = t not in piece and not back
            rest = edges(j, pos + 1)
            if back:
                # the branch back: taken once the row is decoded and nothing the turn is about lies just ahead
                front, near = [e for e in rest if e is not None], False
                for _ in range(8):
                    near = near or any(wanted(blocks[e]) for e in front)
                    front = [e for x in front for e in edges(x, 0) if e is not None]
                take = state["past_wait"] and not near
            elif t_out or rest == [None]:
                take = not t_out                 # one side leaves the hot piece: the other one
            else:
                r_t = reach([order[t]])
                r_f = reach(rest)
                out_t, d_t = side([order[t]], False, r_f)
                out_f, d_f = side(rest, False, r_t)
                if out_t != out_f:
                    take = out_f
                elif "exec" in op:
                    take = op.endswith("execnz")
                elif (d_t is None) != (d_f is None):
                    take = d_f is None
                else:
                    take = d_t is not None and d_t < d_f
            if take:
                nxt = order.get(t)
                break
        path.append(Block(b.name, b.loop, part))
        if state["stored"] and all(o.startswith("s_") for o, _, _ in part):
            state["flushed"] = True              # a block of scalar work only behind a store: the turn has flushed
        if nxt is not None and blocks[nxt].name in latch:
            while nxt < h:                     # the latch in front of the header closes the turn
                path.append(blocks[nxt])
                nxt += 1
            break
        j = nxt
    return path


def analyse_turns(path, rates=None):
    """-> {instance: {turn: dict(whole=mix, slots=mix, tail=mix, rest=mix, blocks=[names], tail_agrees=bool)}}"""
    rates = rates or Rates()
    res = collections.OrderedDict()
    for name, info, blocks, parents in kernels(path):
        head, lb = row_loop(blocks, parents)
        if head is None or not any(_b(o) == "v_mad_i64_i32" for b in lb for o, _, _ in b.ins):
            continue
        tail = row_tail_path(blocks, lb)
        if not tail:
            continue
        reg = regions(lb)
        slot_names = {b.name for r, bs in reg.items() if r.startswith("slot") for b in bs}
        tail_names = {b.name for b in tail}
        res[name] = collections.OrderedDict()
        for turn in TURNS:
            p = turn_path(blocks, lb, turn)
            mine = [b for b in p if b.name in tail_names]
            res[name][turn] = dict(
                whole=mix(p, rates), slots=mix([b for b in p if b.name in slot_names], rates), tail=mix(mine, rates),
                rest=mix([b for b in p if b.name not in slot_names and b.name not in tail_names], rates),
                blocks=[b.name for b in p],
                tail_agrees=[b.name for b in mine] == [b.name for b in tail] and
                [len(b.ins) for b in mine[:-1]] == [len(b.ins) for b in tail[:-1]])
    return res


def vmcnt_waits_beside_mads(loop_blocks):
    """-> [(block name, operands)]: every s_waitcnt that waits for vector memory in a row-loop block that holds a
    v_mad_i64_i32 -- the filter's and the rematrix's multiply-adds must not wait for the chunk or for the PCM stores"""
    out = []
    for b in loop_blocks:
        if any(_b(o) == "v_mad_i64_i32" for o, _, _ in b.ins):
            out += [(b.name, a) for o, a, _ in b.ins if o == "s_waitcnt" and "vmcnt" in a]
    return out


def sgpr_pair_selects(blocks_):
    """-> [(block name, operands)]: v_cndmask_b32_e64 whose mask is an SGPR pair"""
    return [(b.name, a) for b in blocks_ for o, a, _ in b.ins
            if o == "v_cndmask_b32_e64" and re.search(r",\s*s\[\d+:\d+\]\s*$", a)]


def analyse_row_tail(path, rates=None):
    """-> {instance name: dict(mix of the row tail's path, + path=[Block], vmcnt_beside_mads, sgpr_selects)} for every
    instance with a rematrix (the chain parse pass has none)"""
    rates = rates or Rates()
    res = collections.OrderedDict()
    for name, info, blocks, parents in kernels(path):
        head, lb = row_loop(blocks, parents)
        if head is None or not any(_b(o) == "v_mad_i64_i32" for b in lb for o, _, _ in b.ins):
            continue
        tail = row_tail_path(blocks, lb)
        m = mix(tail, rates)
        m.update(path=tail, vmcnt_beside_mads=vmcnt_waits_beside_mads(lb), sgpr_selects=sgpr_pair_selects(tail))
        res[name] = m
    return res


def mix(blocks_, rates):
    """-> dict(total, valu, fast, slow, unclassified, cycles, hist, scratch, lane_moves)"""
    h, cls, unc = collections.Counter(), collections.Counter(), set()
    for b in blocks_:
        for op, operands, _ in b.ins:
            h[_b(op)] += 1
            if op.startswith("v_"):
                cls[rates.classify(op, operands)] += 1
                if rates.classify(op, operands) == "unclassified":
                    unc.add(_b(op))
    valu = sum(cls.values())
    return dict(total=sum(h.values()), valu=valu, fast=cls["fast"], slow=cls["slow"], unclassified=cls["unclassified"],
                cycles=cls["fast"] * rates.fast_cycles + (cls["slow"] + cls["unclassified"]) * rates.slow_cycles,
                hist=h, unclassified_ops=unc, scratch=sum(n for o, n in h.items() if o.startswith("scratch_")),
                lane_moves=h["v_readlane_b32"] + h["v_writelane_b32"])


def analyse(path, rates=None):
    """-> [(instance name, info, row-loop header, OrderedDict region -> mix, whole-loop mix)]"""
    rates = rates or Rates()
    res = []
    for name, info, blocks, parents in kernels(path):
        head, lb = row_loop(blocks, parents)
        if head is None:
            continue
        reg = regions(lb)
        res.append((name, info, head, collections.OrderedDict((r, mix(bs, rates)) for r, bs in reg.items()), mix(lb, rates)))
    return res


def report(path, out=sys.stdout):
    rates = Rates()
    w = out.write
    w("compiler: %s\n" % compiler_version())
    w("classes from profiles/r05_valu_issue_rates.txt, 2 waves per SIMD: threshold %.2f ns; fast %.2f cycles, slow %.2f cycles"
      " at %.1f GHz; unclassified opcodes are priced as slow\n" % (rates.threshold, rates.fast_cycles, rates.slow_cycles,
                                                                     rates.clock_ghz))
    for name, info, head, reg, whole in analyse(path, rates):
        w("\n== %s%s\n" % (name, "   (the headline instance)" if name == HEADLINE else ""))
        w("   VGPRs %s, occupancy %s, scratch %s B (whole kernel), LDS %s B; row loop at %s: %d instructions, "
          "scratch_ in the loop %d, v_readlane/v_writelane in the loop %d\n" %
          (info.get("NumVgprs"), info.get("Occupancy"), info.get("ScratchSize"), info.get("LDSByteSize"), head,
           whole["total"], whole["scratch"], whole["lane_moves"]))
        w("   %-20s %6s %6s %6s %6s %7s %10s\n" % ("region", "instr", "VALU", "fast", "slow", "unclass", "w.cycles"))
        for r, m in list(reg.items()) + [("whole row loop", whole)]:
            w("   %-20s %6d %6d %6d %6d %7d %10.0f\n" % (r, m["total"], m["valu"], m["fast"], m["slow"], m["unclassified"],
                                                        m["cycles"]))
        for r, m in reg.items():
            if r.startswith("slot 1") or r == "slots 0-1" or (r == "slot 0" and "slot 1" not in reg):
                w("   %s: %s\n" % (r, ", ".join("%s %d" % (o, n) for o, n in m["hist"].most_common())))
        w("   whole row loop, VALU: %s\n" % ", ".join("%s %d" % (o, n) for o, n in whole["hist"].most_common() if o.startswith("v_")))
        w("   unclassified: %s\n" % (", ".join(sorted(whole["unclassified_ops"])) or "none"))
    w("\n== row tail: the path from behind the last slot to the hand-written wait for the chunk (cold branches left out)\n")
    w("   %-52s %6s %6s %6s %6s %7s %10s %8s %8s\n" % ("instance", "instr", "VALU", "fast", "slow", "unclass", "w.cycles",
                                                       "vmwaits", "selects"))
    tails = analyse_row_tail(path, rates)
    for name, m in tails.items():
        if not m["path"]:
            w("   %-52s (no such path: the sequential pass rematrixes at the end of an access unit)\n" % name)
            continue
        w("   %-52s %6d %6d %6d %6d %7d %10.0f %8d %8d\n" % (name, m["total"], m["valu"], m["fast"], m["slow"],
                                                            m["unclassified"], m["cycles"], len(m["vmcnt_beside_mads"]),
                                                            len(m["sgpr_selects"])))
    w("   (vmwaits: s_waitcnt vmcnt in a row-loop block that holds v_mad_i64_i32; selects: v_cndmask_b32_e64 on an SGPR pair "
      "in the path)\n")
    if HEADLINE in tails:
        w("   headline, VALU: %s\n" % ", ".join("%s %d" % (o, n) for o, n in tails[HEADLINE]["hist"].most_common()
                                                 if o.startswith("v_")))
    report_rest(path, rates, out)


def report_rest(path, rates, out):
    """the row loop outside the slots and the row tail: "other" by sub-region (static), and the three kinds of turn"""
    w = out.write
    turns = analyse_turns(path, rates)
    w("\n== the rest of the row loop: \"other\" and the latch in front of the header, by sub-region (static counts)\n")
    for name, info, blocks, parents in kernels(path):
        head, lb = row_loop(blocks, parents)
        if name not in turns or not all(t["tail_agrees"] for t in turns[name].values()):
            continue
        w("   %s\n" % name)
        w("   %-34s %6s %6s %6s %6s %7s %10s\n" % ("sub-region", "instr", "VALU", "fast", "slow", "unclass", "w.cycles"))
        for r, bs in rest_regions(blocks, lb).items():
            m = mix(bs, rates)
            w("   %-34s %6d %6d %6d %6d %7d %10.0f\n" % (r, m["total"], m["valu"], m["fast"], m["slow"], m["unclassified"],
                                                        m["cycles"]))
    w("\n== turns: what a lockstep wave executes from the loop's header to the branch back (cold branches left out), and the\n"
      "   part of it outside the slots, the slot masks and the row tail (\"rest\")\n")
    w("   %-52s %-7s %6s %6s | %6s %6s %6s %6s %7s %10s\n" % ("instance", "turn", "instr", "VALU", "rest", "VALU", "fast", "slow",
                                                            "unclass", "w.cycles"))
    for name, t in turns.items():
        if not all(d["tail_agrees"] for d in t.values()):
            w("   %-52s (no walk: the row tail is not met on the way -- two substreams a lane)\n" % name)
            continue
        for turn in TURNS:
            d, r = t[turn]["whole"], t[turn]["rest"]
            w("   %-52s %-7s %6d %6d | %6d %6d %6d %6d %7d %10.0f\n" % (name, turn, d["total"], d["valu"], r["total"], r["valu"],
                                                                       r["fast"], r["slow"], r["unclassified"], r["cycles"]))
        p, f, x = (t[k]["rest"] for k in TURNS)
        for share, label in ((0.25, "1/4"), (0.2, "1/5")):
            w("   %-52s per row, refill share %s, flush 1/4: rest VALU %.1f, w.cycles %.0f\n" % (
                "", label, p["valu"] + share * (f["valu"] - p["valu"]) + 0.25 * (x["valu"] - p["valu"]),
                p["cycles"] + share * (f["cycles"] - p["cycles"]) + 0.25 * (x["cycles"] - p["cycles"])))
    if HEADLINE in turns:
        for turn in TURNS:
            d = turns[HEADLINE][turn]
            w("   headline, %s turn walks: %s\n" % (turn, " ".join(d["blocks"])))
            w("   headline, %s turn, rest VALU: %s\n" % (turn, ", ".join(
                "%s %d" % (o, n) for o, n in d["rest"]["hist"].most_common() if o.startswith("v_"))))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else compile_asm()
    report(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
