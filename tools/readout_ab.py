"""A/B of reading the solution back: ADVANCES coupling intervals ("advances") of STEPS fused forward-Euler steps each
(rdyhip_euler_step at a fixed dt, F never stored), with the owned-cell heights wanted on the host after every advance, in
three forms --

  a  steps   the steps alone, nothing read (what the other forms add to)
  b  whole   what a host does today after each advance: a blocking copy of the whole [num_cells][3] state to the host
             (VecGetArrayRead of a Vec placed on a device array) and a host loop that picks h (RDyGetOwnedCellHeights,
             src/rdydata.c:171-181); the device is drained and idle meanwhile
  c  planes  rdyhip_state_read_begin(H) behind each advance's last step, and rdyhip_state_read_wait + rdyhip_state_read_get once
             the NEXT advance's steps are enqueued (the last advance's read is collected at the end, inside the timed window)

All forms run in ONE process, interleaved round by round (a b c a b c ...).  A round of a form is timed with the host clock from
a drained device to a drained device: forms b and c do host work (the copy into pageable memory, the picking loop, the copy out
of pinned memory) that device events would not see.  ms per advance = the round / ADVANCES; median over the rounds and their
spread (max - min) / median.  The claim under test: (c - a) < (b - a) at every size by more than that spread; the numbers are
written down whatever they are, and `claim` says per size whether it held.  The heights of the last round of b and c are
compared bit for bit.

Then, per size, with device events around LAUNCHES back-to-back launches: state_planes_kernel for one and for three components
against axpy_owned_kernel (rdyhip_axpy_owned), next to its byte ratio (24 + 8 k) / 72, and the two launches + the 80-byte copy of
rdyhip_error_sums.

Sizes: 0.36 M, 1 M and 10 M triangles (flat-bed dam break, the state of BASELINE.json configs[1]), first order.

usage (GPU box): python tools/readout_ab.py [--out FILE] [--rounds R] [--advances A] [--steps K] [--only TAG,TAG] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("0.36M", 600, 300), ("1M", 1000, 500), ("10M", 2500, 2000)]
SMALL = [("small", 60, 32)]      # rehearsal of the tool itself, not a measurement
FORMS = ("steps", "whole", "planes")
LAUNCHES = 50


def rounds_of(case, op, rounds, advances, steps):
    """`rounds` x FORMS; ({form: [ms per advance of each round]}, the heights of b and c after the last advance are the same bits)"""
    import torch
    from rdycore_amd.operator import COMPONENT_H
    mesh = case.mesh
    no, dt = mesh.num_owned_cells, case.dt
    own = np.asarray(mesh.cell_owned_to_local)
    u0 = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    cur0, nxt0 = u0.clone(), u0.clone()
    host = torch.empty((mesh.num_cells, 3), dtype=torch.float64)          # pageable, as a Vec's host array
    host_np = host.numpy()
    h = np.empty(no)
    ms = {form: [] for form in FORMS}
    kept = {}
    for r in range(-1, rounds):                   # round -1: warm-up of every form (code objects, first-use allocations), not counted
        for form in FORMS:
            cur, nxt = cur0, nxt0
            cur.copy_(u0)
            nxt.copy_(u0)
            heights = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for adv in range(advances):
                for _ in range(steps):
                    op.euler_step(dt, cur, nxt)
                    cur, nxt = nxt, cur
                if form == "whole":
                    host.copy_(cur)                                       # blocking: the whole state crosses, the device drains
                    np.take(host_np[:, 0], own, out=h)                    # the getter's loop
                    heights.append(h.copy())
                elif form == "planes":
                    if adv > 0:
                        heights.append(op.read_state(COMPONENT_H))        # the previous advance's, behind this advance's enqueued steps
                    op.read_state_begin(cur, COMPONENT_H)
            if form == "planes":
                heights.append(op.read_state(COMPONENT_H))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= 0:
                ms[form].append((t1 - t0) * 1e3 / advances)
            kept[form] = heights
    same = len(kept["whole"]) == len(kept["planes"]) == advances and all(
        np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(kept["whole"], kept["planes"]))
    return ms, bool(same)


def kernel_times(case, op):
    """us per launch: axpy_owned_kernel, state_planes_kernel with 1 and 3 components, rdyhip_error_sums (two launches + 80-byte copy)"""
    import torch
    mesh = case.mesh
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f = torch.zeros((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    out = torch.empty((3, mesh.num_owned_cells), dtype=torch.float64, device="cuda")
    calls = {"axpy": lambda: op.axpy_owned(0.0, f, u), "planes1": lambda: op.state_planes(u, 1, out=out),
             "planes3": lambda: op.state_planes(u, 7, out=out)}
    us = {}
    for name, call in calls.items():
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            call()
        e1.record()
        torch.cuda.synchronize()
        us[name] = e0.elapsed_time(e1) * 1e3 / LAUNCHES
    # the error sums: enqueue LAUNCHES calls through the C ABI without reading any result, then one get
    from rdycore_amd import _lib
    from rdycore_amd.operator import _ptr, _stream
    lib = _lib.load()
    op.error_sums(u)                         # first use: the areas and records are allocated
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        _lib.check(lib.rdyhip_error_sums(op._h, _ptr(u), None, _stream()))
    e1.record()
    torch.cuda.synchronize()
    us["error_sums"] = e0.elapsed_time(e1) * 1e3 / LAUNCHES
    return us


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--advances", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds of each form")
    if args.advances < 2:
        raise SystemExit("at least two advances per round (a read is collected behind the next advance's steps)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readout_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    sizes = [s for s in (SMALL if args.small else SIZES) if not args.only or s[0] in args.only.split(",")]
    lines = [f"# tools/readout_ab.py: {args.rounds} interleaved rounds of {args.advances} advances of {args.steps} fused Euler steps per form; "
             f"device: {torch.cuda.get_device_name(0)}"]
    result = {}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# ms per advance, host clock from a drained device to a drained device, median over the rounds (spread = (max - min) / median)")
    say("# a = the steps alone; b = + blocking copy of the whole state and a host loop picking h; c = + rdyhip_state_read_begin(H),")
    say("# wait + get behind the next advance's enqueued steps.  claim: (c - a) < (b - a) by more than the largest spread, in ms")
    say(f"{'case':<8}{'cells':>10}{'a ms':>10}{'spread':>8}{'b ms':>10}{'spread':>8}{'c ms':>10}{'spread':>8}{'b - a':>10}{'c - a':>10}{'noise ms':>10}"
        f"  claim  same bits")
    kern = {}
    for tag, nx, ny in sizes:
        case = CS.dam_break_case(M.structured_tri_mesh(nx, ny, 1.0, order="tiled"), float(nx), dt=1e-3)
        op = CS.create_operator(case)
        ms, same = rounds_of(case, op, args.rounds, args.advances, args.steps)
        m = {form: med_spread(ms[form]) for form in FORMS}
        a, b, c = (m[form][0] for form in FORMS)
        noise = max(m[form][0] * m[form][1] for form in FORMS)
        claim = (b - a) - (c - a) > noise
        kern[tag] = kernel_times(case, op)
        result[tag] = {"cells": case.mesh.num_owned_cells, "same_bits": same, "claim_holds": bool(claim), "noise_ms": noise,
                       **{f"{k}_ms": m[k][0] for k in FORMS}, **{f"{k}_spread": m[k][1] for k in FORMS}, **{f"{k}_rounds_ms": ms[k] for k in FORMS},
                       **{f"{k}_us": v for k, v in kern[tag].items()}}
        say(f"{tag:<8}{case.mesh.num_owned_cells:>10}{a:>10.3f}{m['steps'][1]:>8.3f}{b:>10.3f}{m['whole'][1]:>8.3f}{c:>10.3f}{m['planes'][1]:>8.3f}"
            f"{b - a:>10.3f}{c - a:>10.3f}{noise:>10.3f}  {str(bool(claim)):<5}  {same}")
        op.destroy()
        del op, case
    say(f"# us per launch, device events around {LAUNCHES} back-to-back launches: axpy_owned_kernel (72 B/cell), state_planes_kernel with k = 1 and")
    say("# k = 3 components ((24 + 8 k) B/cell: byte ratio 0.444 and 0.667), rdyhip_error_sums (two launches + the 80-byte copy)")
    say(f"{'case':<8}{'axpy us':>10}{'k=1 us':>10}{'/ axpy':>8}{'k=3 us':>10}{'/ axpy':>8}{'sums us':>10}")
    for tag, _, _ in sizes:
        k = kern[tag]
        say(f"{tag:<8}{k['axpy']:>10.1f}{k['planes1']:>10.1f}{k['planes1'] / k['axpy']:>8.3f}{k['planes3']:>10.1f}{k['planes3'] / k['axpy']:>8.3f}"
            f"{k['error_sums']:>10.1f}")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
