"""A/B of the classical Runge-Kutta step: EulerStepper(temporal="rk4", fused=False) -- the loop of 4 RHS calls, 3 copies and
7 axpy_owned launches -- against fused=True -- rdyhip_rk4_step: 4 RHS launches, 3 rk4_stage_kernel, 1 rk4_combine_kernel.

  step times     both steppers in ONE process on the same operator, interleaved round by round (A B A B ...), each round
                 timed with device events around STEPS steps from the same initial state; median over the rounds and their
                 spread (max - min) / median
  kernel times   a second process under `rocprofv3 --kernel-trace` runs the same rounds; per kernel the mean duration of each
                 round's dispatches, median over the rounds and spread: rk4_stage_kernel and rk4_combine_kernel, in their
                 16-byte and their 8-byte form, against the axpy_owned_kernel launches of the loop they replace, on the same
                 cells
  --counters     two more processes, one per counter (`rocprofv3 --pmc FETCH_SIZE`, then `--pmc WRITE_SIZE`: the hardware
                 collects one of them per pass), over one round of 5 steps: KB per launch that pass the L2's far side

Sizes: 0.36 M, 1 M and 10 M triangles (flat-bed dam break, the state of BASELINE.json configs[1]), first order; second
order (minmod) at 1 M.

usage (GPU box): python tools/rk4_ab.py [--out FILE] [--rounds R] [--steps K] [--only TAG,TAG] [--no-steps] [--no-kernels] [--counters] [--small]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("0.36M", 600, 300, False), ("1M", 1000, 500, False), ("1M_second_order", 1000, 500, True), ("10M", 2500, 2000, False)]
SMALL = [("small", 60, 32, False), ("small_second_order", 60, 32, True)]      # rehearsal of the tool itself, not a measurement
# kernel family -> launches per step of the form that uses it (the loop: 3 stage updates, then 4 for the combination)
KERNELS = {"axpy_owned_kernel": 7, "rk4_stage_kernel<true>": 3, "rk4_stage_kernel<false>": 3, "rk4_combine_kernel<true>": 1, "rk4_combine_kernel<false>": 1}


def make(nx, ny, second_order):
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    case = CS.dam_break_case(M.structured_tri_mesh(nx, ny, 1.0, order="tiled"), float(nx), dt=1e-3)
    case.config.second_order = second_order
    return case, CS.create_operator(case)


def rounds_of(case, op, rounds, steps, timed):
    """`rounds` x (loop, step, step8), each `steps` steps from the initial state; returns {form: [ms per step of each round]}"""
    import torch
    from rdycore_amd.timestep import EulerStepper
    u0 = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    # "step8": the one-call step on a state array that starts 8 bytes into its buffer, which the 16-byte form of the update
    # kernels cannot take: the 8-byte form of both, same bits (an A/B of the access width without a knob)
    u8 = torch.empty(u0.numel() + 1, dtype=torch.float64, device="cuda")[1:].view(u0.shape)
    assert u8.data_ptr() % 16 == 8
    forms = {"loop": (EulerStepper(op, temporal="rk4", fused=False), u0.clone()), "step": (EulerStepper(op, temporal="rk4", fused=True), u0.clone()),
             "step8": (EulerStepper(op, temporal="rk4", fused=True), u8)}
    ms = {k: [] for k in forms}
    for r in range(-1, rounds):                   # round -1: warm-up of both forms (code objects, workspace), not counted
        for name, (st, u) in forms.items():
            u.copy_(u0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.advance(u, case.dt, steps * case.dt)
            e1.record()
            torch.cuda.synchronize()
            if r >= 0 and timed:
                ms[name].append(e0.elapsed_time(e1) / steps)
    same = bool(torch.equal(forms["loop"][1], forms["step"][1])) and bool(torch.equal(forms["loop"][1], forms["step8"][1]))
    return ms, same


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m > 0 else 0.0


def sizes_of(args):
    sizes = SMALL if args.small else SIZES
    return [s for s in sizes if not args.only or s[0] in args.only.split(",")]


def child(args):
    """under rocprofv3: the same rounds, nothing timed here"""
    import torch
    torch.cuda.set_device(0)
    for tag, nx, ny, so in sizes_of(args):
        case, op = make(nx, ny, so)
        rounds_of(case, op, args.rounds, args.steps, timed=False)
        op.destroy()
        print("child done", tag, flush=True)


def traced_child(args, pattern, rounds, steps, extra=()):
    """runs the child under rocprofv3 (with `extra` arguments); the rows of the csv that matches `pattern`"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", *extra, "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "rk4", "--", sys.executable, os.path.abspath(__file__),
                                       "--child", "--rounds", str(rounds), "--steps", str(steps)]
        cmd += (["--small"] if args.small else []) + (["--only", args.only] if args.only else [])
        run = subprocess.run(cmd)               # its output goes where ours goes: a long pass shows that it is alive
        if run.returncode != 0:
            raise SystemExit(f"the traced run failed ({run.returncode})")
        files = glob.glob(os.path.join(tmp, "**", pattern), recursive=True)
        if not files:
            raise RuntimeError(f"no {pattern} under {tmp}")
        with open(files[0]) as fh:
            return list(csv.DictReader(fh))


def family(name):
    return next((k for k in KERNELS if k in name), None)


def by_size_and_round(seq, sizes, rounds, steps):
    """The dispatches are in a known order: per size, a warm-up round and `rounds` rounds of `steps` steps.
    seq: {family: [value per dispatch, in dispatch order]} -> {size: {family: [[values of a round]]}}"""
    out = {}
    for i, (tag, _, _, _) in enumerate(sizes):
        out[tag] = {}
        for k, n in KERNELS.items():
            block = n * steps * (rounds + 1)
            mine = seq[k][i * block:(i + 1) * block]
            if len(mine) != block:
                raise RuntimeError(f"{tag}: {len(mine)} dispatches of {k}, expected {block}")
            out[tag][k] = [mine[(r + 1) * n * steps:(r + 2) * n * steps] for r in range(rounds)]
    return out


def kernel_table(rows, sizes, rounds, steps):
    """rows: [(start ns, family, duration ns)] -> {size: {family: (median us, spread)}}"""
    rows = sorted(rows)
    split = by_size_and_round({k: [d for _, f, d in rows if f == k] for k in KERNELS}, sizes, rounds, steps)
    out = {}
    for tag, fams in split.items():
        res = {k: med_spread([statistics.mean(x) / 1e3 for x in per_round]) for k, per_round in fams.items()}
        ax = fams["axpy_owned_kernel"]        # by position in the step: the three stage updates / the four of the combination
        res["axpy_at_stage_updates"] = med_spread([statistics.mean(d for j, d in enumerate(x) if j % 7 < 3) / 1e3 for x in ax])
        res["axpy_at_combination"] = med_spread([statistics.mean(d for j, d in enumerate(x) if j % 7 >= 3) / 1e3 for x in ax])
        out[tag] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--small", action="store_true", help="two tiny meshes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rk4_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    sizes = sizes_of(args)
    lines = [f"# tools/rk4_ab.py: {args.rounds} interleaved rounds of {args.steps} steps per form; device: {torch.cuda.get_device_name(0)}"]
    result = {"steps": {}, "kernels": {}, "counters": {}}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if not args.no_steps:
        say("# step: ms per Runge-Kutta step, median over the rounds (spread = (max - min) / median of the rounds); step8 = the one-call step")
        say("# with the 8-byte form of its update kernels (state array 8 bytes into its buffer)")
        say(f"{'case':<18}{'cells':>10}{'loop ms':>10}{'spread':>8}{'step ms':>10}{'spread':>8}{'step/loop':>10}{'step8 ms':>10}{'spread':>8}{'step8/loop':>11}  same bits")
        for tag, nx, ny, so in sizes:
            case, op = make(nx, ny, so)
            ms, same = rounds_of(case, op, args.rounds, args.steps, timed=True)
            (ml, sl), (mf, sf), (m8, s8) = med_spread(ms["loop"]), med_spread(ms["step"]), med_spread(ms["step8"])
            result["steps"][tag] = {"cells": case.mesh.num_owned_cells, "loop_ms": ml, "loop_spread": sl, "step_ms": mf, "step_spread": sf,
                                    "step8_ms": m8, "step8_spread": s8, "same_bits": same}
            say(f"{tag:<18}{case.mesh.num_owned_cells:>10}{ml:>10.4f}{sl:>8.3f}{mf:>10.4f}{sf:>8.3f}{mf / ml:>10.3f}{m8:>10.4f}{s8:>8.3f}{m8 / ml:>11.3f}  {same}")
            op.destroy()
    if not args.no_kernels:
        rows = [(int(r["Start_Timestamp"]), family(r.get("Kernel_Name", "")), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                for r in traced_child(args, "*kernel_trace.csv", args.rounds, args.steps)]
        table = kernel_table([r for r in rows if r[1]], sizes, args.rounds, args.steps)
        result["kernels"] = table
        say("# kernels: us per launch (rocprofv3 --kernel-trace, a run of its own), median over the rounds of the round means (spread as above);")
        say("# axpy = the 7 axpy_owned_kernel launches per step of the loop, on the same cells (at its 3 stage updates / its 4 of the combination);")
        say("# stage16 / stage8, comb16 / comb8: the 16-byte and 8-byte forms; bounds: stage <= axpy, combine <= 2 x axpy")
        say(f"{'case':<18}{'axpy us':>9}{'spread':>8}{'(stage':>8}{'comb.)':>8}{'stage16':>9}{'spread':>8}{'/axpy':>7}{'stage8':>9}{'/axpy':>7}"
            f"{'comb16':>9}{'spread':>8}{'/axpy':>7}{'comb8':>9}{'/axpy':>7}")
        for tag, r in table.items():
            a = r["axpy_owned_kernel"]
            s16, s8, c16, c8 = (r[k] for k in ("rk4_stage_kernel<true>", "rk4_stage_kernel<false>", "rk4_combine_kernel<true>", "rk4_combine_kernel<false>"))
            say(f"{tag:<18}{a[0]:>9.2f}{a[1]:>8.3f}{r['axpy_at_stage_updates'][0]:>8.2f}{r['axpy_at_combination'][0]:>8.2f}{s16[0]:>9.2f}{s16[1]:>8.3f}"
                f"{s16[0] / a[0]:>7.3f}{s8[0]:>9.2f}{s8[0] / a[0]:>7.3f}{c16[0]:>9.2f}{c16[1]:>8.3f}{c16[0] / a[0]:>7.3f}{c8[0]:>9.2f}{c8[0] / a[0]:>7.3f}")
    if args.counters:
        c_rounds, c_steps = 1, 5      # counting serialises the dispatches, and a count does not vary as a time does
        say("# counters: KB per launch (rocprofv3 --pmc, one counter per pass, each pass a run of its own), mean over one round of 5 steps;")
        say("# algorithmic = 72 B per cell (stage, axpy), 144 B (combine)")
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            recs = traced_child(args, "*counter_collection.csv", c_rounds, c_steps, extra=("--pmc", ctr))
            recs.sort(key=lambda r: int(r.get("Dispatch_Id", 0)))
            seq = {k: [float(r["Counter_Value"]) for r in recs if r.get("Counter_Name") == ctr and family(r.get("Kernel_Name", "")) == k] for k in KERNELS}
            for tag, fams in by_size_and_round(seq, sizes, c_rounds, c_steps).items():
                for k, per_round in fams.items():
                    x = per_round[0]
                    c = result["counters"].setdefault(tag, {}).setdefault(k, {})
                    c[ctr] = statistics.mean(x)
                    if k == "axpy_owned_kernel":
                        c[ctr + "_at_stage_updates"] = statistics.mean(v for j, v in enumerate(x) if j % 7 < 3)
                        c[ctr + "_at_combination"] = statistics.mean(v for j, v in enumerate(x) if j % 7 >= 3)
        say(f"{'case':<18}{'kernel':<34}{'FETCH_SIZE':>12}{'WRITE_SIZE':>12}{'algorithmic KB':>16}")
        cells = {tag: 2 * nx * ny for tag, nx, ny, _ in sizes}
        for tag, fams in result["counters"].items():
            for k, c in fams.items():
                alg = cells[tag] * (144 if "combine" in k else 72) / 1024
                say(f"{tag:<18}{k:<34}{c['FETCH_SIZE']:>12.0f}{c['WRITE_SIZE']:>12.0f}{alg:>16.0f}")
                if k == "axpy_owned_kernel":
                    for pos in ("_at_stage_updates", "_at_combination"):
                        say(f"{tag:<18}{'  axpy' + pos:<34}{c['FETCH_SIZE' + pos]:>12.0f}{c['WRITE_SIZE' + pos]:>12.0f}{alg:>16.0f}")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
