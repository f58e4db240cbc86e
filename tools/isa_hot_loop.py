"""Instruction mix of one kernel per BASIC BLOCK of a hipcc -S dump, and the totals of its hot loop:

    python tools/isa_hot_loop.py file.s <kernel-name-substring> [--cold LABEL,LABEL,...]

One line per block: label, fp64 arithmetic, other VALU, lane ops (v_readlane_b32 / v_writelane_b32: restores and saves of SGPRs
spilled to VGPR lanes), LDS, vector memory, SALU (scalar loads counted apart as SMEM), waits, and the block's branches and
barriers.  A block starts at a label or behind a branch and ends at the next one.

The hot loop is the outermost loop that holds a barrier (the tile loop of the tiled kernels): the blocks from the target of the
widest backward branch that spans an s_barrier (the loop head) to that branch (the back edge), marked `*`.  The totals are
STATIC: every block of the loop once, the edge rounds of the tiled kernels (a loop nested in it, run twice per tile) too.  The
tool cannot know which lanes are live, so blocks the hot path never runs (boundary edges, the Courant tie path, the
INTERIOR-phase tile search, the o2l and src_mom arms) are in the totals unless they are named with --cold; the per-block lines
say where the instructions sit.  isa_phases.py cuts at barriers only and mixes the code outside the loop in as well.

As a module: blocks(), hot_loop() and totals() return the same numbers (tests/test_hot_loop_cpu.py)."""
import collections
import re
import sys

CLASSES = ("fp64", "valu", "lane", "lds", "vmem", "smem", "salu", "wait")
LANE_OPS = ("v_readlane_b32", "v_writelane_b32")


def classify(op):
    if op in LANE_OPS: return "lane"
    if op.startswith("v_") and "f64" in op: return "fp64"
    if op.startswith("v_"): return "valu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    if op == "s_waitcnt": return "wait"
    if op.startswith(("s_load_", "s_buffer_load_")): return "smem"
    if op.startswith(("s_cbranch", "s_branch", "s_barrier", "s_nop", "s_endpgm", "s_setprio", "s_sleep")): return None
    if op.startswith("s_"): return "salu"
    return None


class Block:
    def __init__(self, label, index):
        self.label, self.index = label, index
        self.counts = collections.Counter()
        self.ops = collections.Counter()
        self.branches, self.barriers = [], 0


def kernel_body(lines, pat):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S+:", l) and pat in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def blocks(lines, pat):
    """The kernel's basic blocks in program order."""
    out = [Block("entry", 0)]
    anon = 0
    fresh = False  # the previous instruction was a branch: the next one opens a block even without a label
    for l in kernel_body(lines, pat):
        t = l.split(";")[0].strip()
        if not t or t.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", t)
            if not m:
                continue
            if out[-1].counts or out[-1].branches or out[-1].barriers or out[-1].label != "entry":
                out.append(Block(m.group(1), len(out)))
            else:
                out[-1].label = m.group(1)
            fresh = False
            continue
        if t.endswith(":"):
            continue
        if fresh:
            anon += 1
            out.append(Block(f"{out[-1].label.split('+')[0]}+{anon}", len(out)))
            fresh = False
        op = t.split()[0]
        b = out[-1]
        b.ops[op] += 1
        c = classify(op)
        if c:
            b.counts[c] += 1
        if op == "s_barrier":
            b.barriers += 1
        if op.startswith(("s_cbranch", "s_branch")):
            b.branches.append((op, t.split()[-1]))
            fresh = True
    return out


def hot_loop(bl):
    """(head index, back-edge index) of the outermost loop that holds a barrier"""
    at = {b.label: b.index for b in bl}
    best = None
    loops = []
    for b in bl:
        for _, target in b.branches:
            if target in at and at[target] <= b.index:
                loops.append((at[target], b.index))
    for head, back in loops:
        if any(x.barriers for x in bl[head:back + 1]) and (best is None or back - head > best[1] - best[0]):
            best = (head, back)
    if best is None:
        raise SystemExit("no loop with a barrier in this kernel")
    return best


def totals(bl, head, back, cold=()):
    tot = collections.Counter()
    for b in bl[head:back + 1]:
        if b.label in cold:
            continue
        for c in CLASSES:
            tot[c] += b.counts[c]
    return tot


def static_ops(lines, pat, ops=LANE_OPS):
    """Whole-kernel static count of the given opcodes."""
    return sum(b.ops[o] for b in blocks(lines, pat) for o in ops)


def loop_code(lines, pat):
    """The hot loop's instructions in program order (labels and directives dropped)."""
    body = kernel_body(lines, pat)
    bl = blocks(lines, pat)
    head, back = hot_loop(bl)
    first = next(i for i, l in enumerate(body) if l.startswith(bl[head].label + ":"))
    after = bl[back + 1].label if back + 1 < len(bl) and bl[back + 1].label.startswith(".LBB") else None
    last = next((i for i, l in enumerate(body) if after and l.startswith(after + ":")), len(body))
    code = [l.split(";")[0].strip() for l in body[first:last]]
    return [t for t in code if t and not t.startswith(".") and not t.endswith(":")]


def lds_round_trips(code):
    """s_waitcnt instructions that carry an lgkmcnt and have at least one ds_read issued since the previous such wait: the LDS
    round trips a wave pays one after the other on a stretch of code (static, cold arms included)."""
    n, pending = 0, False
    for t in code:
        op = t.split()[0]
        if op.startswith("ds_read"):
            pending = True
        elif op == "s_waitcnt" and "lgkmcnt" in t:
            n += pending
            pending = False
    return n


def phase2_round_trips(lines, pat):
    """LDS round trips of phase 2's reads: from the hot loop's second s_barrier to the first hinted global_load behind it (the
    next tile's per-cell streams, issued when the cell sum and the cell's results are done)."""
    code = loop_code(lines, pat)
    bars = [i for i, t in enumerate(code) if t.split()[0] == "s_barrier"]
    start = bars[1]
    end = next(i for i in range(start, len(code)) if code[i].startswith("global_load") and re.search(r"\bnt\b", code[i]))
    return lds_round_trips(code[start:end])


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    cold = ()
    for i, a in enumerate(argv):
        if a == "--cold": cold = tuple(argv[i + 1].split(",")); args.remove(argv[i + 1])
    lines = open(args[0]).read().split("\n")
    bl = blocks(lines, args[1])
    head, back = hot_loop(bl)
    print(f"{'block':14s} " + " ".join(f"{c:>5s}" for c in CLASSES) + "  branches / barriers")
    for b in bl:
        mark = " " if not head <= b.index <= back else ("c" if b.label in cold else "*")
        br = " ".join(f"{o.replace('s_cbranch_', '').replace('s_branch', 'jmp')}->{t}" for o, t in b.branches)
        print(f"{mark}{b.label:13s} " + " ".join(f"{b.counts[c]:5d}" for c in CLASSES) + f"  {br}{'  BARRIER' * b.barriers}")
    tot = totals(bl, head, back, cold)
    print(f"hot loop {bl[head].label} .. {bl[back].label} (static, every block once; {len(cold)} cold blocks left out):")
    print("  " + "  ".join(f"{c}={tot[c]}" for c in CLASSES) + f"  all VALU-issued={tot['fp64'] + tot['valu'] + tot['lane']}")
    print(f"whole kernel, static: lane ops={sum(b.counts['lane'] for b in bl)}")


if __name__ == "__main__":
    main(sys.argv[1:])
