"""A/B of the time-averaged output fields: a forward-Euler step (rdyhip_euler_step, F never stored) with the means of the
solution, the primitive variables and the sources kept, in two forms --

  host   the way a host does it without rdyhip_output_mean_*: the primitive-variables pointer taken (every RHS launch stores
         24 B/cell), the source pointer taken (the water-only mode of the source is over), three rdyhip_axpy_owned launches per
         step into local-size arrays of its own
  new    one rdyhip_output_mean_accumulate per step: stores off, water-only mode kept
  none   the step alone, no means kept (what the other forms add to)

  step times     all forms in ONE process, interleaved round by round (none host new none host ...), each round timed with
                 device events around STEPS steps from the same initial state; median over the rounds and their spread
                 (max - min) / median
  kernel times   a second process under `rocprofv3 --kernel-trace` runs the same rounds; per kernel the mean duration of each
                 round's dispatches, median over the rounds and spread: output_accumulate_kernel against the
                 axpy_owned_kernel launches of the host form on the same cells.  By bytes the accumulate launch moves 216 B per
                 cell (three variables, canonical source array) against 72 B of one axpy: the bound is 3.0 x.

Sizes: 0.36 M, 1 M and 10 M triangles (flat-bed dam break, the state of BASELINE.json configs[1]) with a uniform rain, first order.

usage (GPU box): python tools/output_mean_ab.py [--out FILE] [--rounds R] [--steps K] [--only TAG,TAG] [--no-steps] [--no-kernels] [--small]"""
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

SIZES = [("0.36M", 600, 300), ("1M", 1000, 500), ("10M", 2500, 2000)]
SMALL = [("small", 60, 32)]      # rehearsal of the tool itself, not a measurement
FORMS = ("none", "host", "new")
# kernel family -> launches per step of the form that uses it
KERNELS = {"axpy_owned_kernel": 3, "output_accumulate_kernel": 1}
ALL = 7


def make(nx, ny):
    """the case, the host-way operator (both pointers taken) and the new-way operator (accumulators enabled)"""
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    case = CS.dam_break_case(M.structured_tri_mesh(nx, ny, 1.0, order="tiled"), float(nx), dt=1e-3)
    case.ext_src[:, 0] = 1e-6          # rain through the ordinary setter; momentum sources stay +0.0
    case.ext_src[:, 1:] = 0.0
    host, new = CS.create_operator(case), CS.create_operator(case)
    new.enable_output_means(ALL)
    return case, host, new


def rounds_of(case, host, new, rounds, steps, timed):
    """`rounds` x FORMS, each `steps` steps from the initial state; returns ({form: [ms per step of each round]}, same bits)"""
    import torch
    assert case.mesh.num_cells == case.mesh.num_owned_cells       # one rank: a state array is its own [owned][3] view
    dt = case.dt
    u0 = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    pv, src = host.primitive_variables, host.external_sources     # from here on the host operator stores and reads 24 B rows
    assert host.primitive_variables_stored() and not host.source_is_water_only()
    assert not new.primitive_variables_stored() and new.source_is_water_only()
    acc = [torch.zeros_like(u0) for _ in range(3)]
    bufs = {form: (u0.clone(), u0.clone()) for form in FORMS}
    ms = {k: [] for k in FORMS}
    means = {}
    for r in range(-1, rounds):                   # round -1: warm-up of every form (code objects), not counted
        for form in FORMS:
            cur, nxt = bufs[form]
            cur.copy_(u0)
            nxt.copy_(u0)
            for a in acc:
                a.zero_()
            new.reset_output_means(ALL)
            op = host if form == "host" else new
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                op.euler_step(dt, cur, nxt)
                if form == "host":
                    host.axpy_owned(dt, nxt, acc[0])
                    host.axpy_owned(dt, pv, acc[1])
                    host.axpy_owned(dt, src, acc[2])
                elif form != "none":
                    new.accumulate_output_means(ALL, dt, nxt)
                cur, nxt = nxt, cur
            e1.record()
            torch.cuda.synchronize()
            if r >= 0 and timed:
                ms[form].append(e0.elapsed_time(e1) / steps)
            if r == rounds - 1 and form != "none":
                means[form] = [a * (1.0 / sum([dt] * steps)) for a in acc] if form == "host" else [new.output_mean(1 << i)[0] for i in range(3)]
    torch.cuda.synchronize()
    same = all(bool(torch.equal(means["host"][i], means["new"][i])) for i in range(3)) if means else None
    assert new.source_is_water_only() and not new.primitive_variables_stored()
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
    for tag, nx, ny in sizes_of(args):
        case, host, new = make(nx, ny)
        rounds_of(case, host, new, args.rounds, args.steps, timed=False)
        host.destroy()
        new.destroy()
        print("child done", tag, flush=True)


def traced_child(args):
    """runs the child under rocprofv3 --kernel-trace; the rows of its kernel trace"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "mean", "--", sys.executable, os.path.abspath(__file__),
               "--child", "--rounds", str(args.rounds), "--steps", str(args.steps)]
        cmd += (["--small"] if args.small else []) + (["--only", args.only] if args.only else [])
        # its output goes where ours goes: a long pass shows that it is alive.  A limit sized to the work -- per size two
        # operators to build and (rounds + 1) x 3 forms x steps steps of at most a millisecond, well under a minute each even
        # traced -- so that a child that hangs does not hold the card
        limit = 120 + 90 * len(sizes_of(args)) + 0.02 * (args.rounds + 1) * 3 * args.steps * len(sizes_of(args))
        try:
            run = subprocess.run(cmd, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"the traced run did not finish within {limit:.0f} s")
        if run.returncode != 0:
            raise SystemExit(f"the traced run failed ({run.returncode})")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel trace under {tmp}")
        with open(files[0]) as fh:
            return list(csv.DictReader(fh))


def family(name):
    return next((k for k in KERNELS if k in name), None)


def kernel_table(rows, sizes, rounds, steps):
    """rows: [(start ns, family, duration ns)] in any order -> {size: {family: (median us, spread)}}.  The dispatches of a
    family come in a known order: per size, a warm-up round and `rounds` rounds of `steps` steps."""
    rows = sorted(rows)
    seq = {k: [d for _, f, d in rows if f == k] for k in KERNELS}
    out = {}
    for i, (tag, _, _) in enumerate(sizes):
        res = {}
        for k, n in KERNELS.items():
            block = n * steps * (rounds + 1)
            mine = seq[k][i * block:(i + 1) * block]
            if len(mine) != block or len(seq[k]) != block * len(sizes):
                raise RuntimeError(f"{tag}: {len(seq[k])} dispatches of {k} in all, expected {block} per size")
            per_round = [mine[(r + 1) * n * steps:(r + 2) * n * steps] for r in range(rounds)]
            res[k] = med_spread([statistics.mean(x) / 1e3 for x in per_round])
            if k == "axpy_owned_kernel":        # by position in the step: the solution, the primitive variables, the sources
                for j, name in enumerate(("axpy_solution", "axpy_primitive_variables", "axpy_sources")):
                    res[name] = med_spread([statistics.mean(d for q, d in enumerate(x) if q % 3 == j) / 1e3 for x in per_round])
        out[tag] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds of each form")
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("output_mean_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    sizes = sizes_of(args)
    lines = [f"# tools/output_mean_ab.py: {args.rounds} interleaved rounds of {args.steps} steps per form; device: {torch.cuda.get_device_name(0)}"]
    result = {"steps": {}, "kernels": {}}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if not args.no_steps:
        say("# step: ms per forward-Euler step with the three means kept, median over the rounds (spread = (max - min) / median of the rounds)")
        say("# none = the step alone; host = pointers taken + 3 axpy_owned; new = one accumulate launch; added = what a form costs on top of the step alone")
        say(f"{'case':<8}{'cells':>10}{'none ms':>10}{'spread':>8}{'host ms':>10}{'spread':>8}{'new ms':>10}{'spread':>8}{'new/host':>10}{'added host':>12}{'added new':>11}"
            f"  same bits")
        for tag, nx, ny in sizes:
            case, host, new = make(nx, ny)
            ms, same = rounds_of(case, host, new, args.rounds, args.steps, timed=True)
            m = {k: med_spread(v) for k, v in ms.items()}
            result["steps"][tag] = {"cells": case.mesh.num_owned_cells, "same_bits": same, **{f"{k}_ms": m[k][0] for k in FORMS},
                                    **{f"{k}_spread": m[k][1] for k in FORMS}}
            say(f"{tag:<8}{case.mesh.num_owned_cells:>10}{m['none'][0]:>10.4f}{m['none'][1]:>8.3f}{m['host'][0]:>10.4f}{m['host'][1]:>8.3f}{m['new'][0]:>10.4f}"
                f"{m['new'][1]:>8.3f}{m['new'][0] / m['host'][0]:>10.3f}{m['host'][0] - m['none'][0]:>12.4f}{m['new'][0] - m['none'][0]:>11.4f}  {same}")
            host.destroy()
            new.destroy()
    if not args.no_kernels:
        rows = [(int(r["Start_Timestamp"]), family(r.get("Kernel_Name", "")), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in traced_child(args)]
        table = kernel_table([r for r in rows if r[1]], sizes, args.rounds, args.steps)
        result["kernels"] = table
        say("# kernels: us per launch (rocprofv3 --kernel-trace, a run of its own), median over the rounds of the round means (spread as above);")
        say("# axpy = the 3 axpy_owned_kernel launches per step of the host form, on the same cells (of the solution / the primitive variables / the sources);")
        say("# acc: output_accumulate_kernel, all three variables; bound: acc <= 3.0 x axpy (216 B against 72 B per cell); TB/s = those bytes over the time")
        say(f"{'case':<8}{'axpy us':>9}{'spread':>8}{'(sol.':>8}{'pv':>8}{'src)':>8}{'TB/s':>7}{'acc us':>9}{'spread':>8}{'/axpy':>7}{'TB/s':>7}")
        cells = {tag: 2 * nx * ny for tag, nx, ny in sizes}
        for tag, r in table.items():
            a, w = r["axpy_owned_kernel"], r["output_accumulate_kernel"]
            say(f"{tag:<8}{a[0]:>9.2f}{a[1]:>8.3f}{r['axpy_solution'][0]:>8.2f}{r['axpy_primitive_variables'][0]:>8.2f}{r['axpy_sources'][0]:>8.2f}"
                f"{72e-6 * cells[tag] / a[0]:>7.2f}{w[0]:>9.2f}{w[1]:>8.3f}{w[0] / a[0]:>7.3f}{216e-6 * cells[tag] / w[0]:>7.2f}")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
