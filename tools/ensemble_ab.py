"""A/B of one ensemble evaluation against the only way to evaluate B members without it: B operators on the same mesh and B
back-to-back rdyhip_rhs_function calls, one per member.

  ens     one rdyhip_ensemble_rhs_function on one operator with B members (ensemble_rhs_kernel, one launch)
  tiled   B rdyhip_rhs_function calls on B operators, the default tiled kernel
  cell    the same with RDYHIP_KERNEL=cell (swe_rhs_kernel, the form the ensemble kernel is built on)

All forms run in ONE process on the same member states, interleaved round by round (ens tiled cell ens tiled cell ...); a round of
a form is LAUNCHES evaluations of all B members between two device events, after a warm-up round of every form.  us per
evaluation of all B members = the round / LAUNCHES; median over the rounds and their spread (max - min) / median.  The F of the
ensemble launch is compared with the cell operators' (largest relative difference; 0 = the same bits).  Beside the times: the
device bytes of the one ensemble operator against those of B operators (rdyhip_layout_info), and the member groups the launch ran
with.  There is no threshold: the numbers are written down whatever they are.

Workload: the flat-bed dam break (BASELINE.json configs[1]) at 0.36 M and 1 M triangles, member m with Manning's n
0.015 (1 + m / 32), dt = 1e-3 (1 + m / 128) and its own perturbation of the momentum; B = 2, 8, 32.  The B operators of the
baselines are created once per size, for the largest B, and the smaller counts use the first B of them.

The group rule is two constants of the library (ENSEMBLE_MIN_WORKGROUPS, ENSEMBLE_MAX_PER_GROUP in csrc/ensemble_kernels.h).  This
tool cannot read them from the library: the `groups` column is computed here from --min-workgroups / --max-per-group, whose
defaults are the library's constants.  Another rule is measured by building a second library with the constants changed and
running this tool under RDYHIP_LIB with the matching options: the column then says what the caller stated, and the output's
first line records it.

usage (GPU box): python tools/ensemble_ab.py [--out FILE] [--rounds R] [--only TAG,TAG] [--members 2,8,32] [--min-workgroups N] [--max-per-group P] [--small]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("0.36M", 600, 300), ("1M", 1000, 500)]
SMALL = [("small", 60, 32)]      # rehearsal of the tool itself, not a measurement
FORMS = ("ens", "tiled", "cell")
LAUNCHES = 50


def member_case(CS, mesh, nx, m):
    case = CS.dam_break_case(mesh, float(nx), dt=1e-3 * (1.0 + m / 128.0), seed=12345 + m)
    case.mannings = np.full(mesh.num_owned_cells, 0.015 * (1.0 + m / 32.0))
    return case


def operators(CS, cases, kernel):
    """one operator per member under RDYHIP_KERNEL=`kernel` (None: the default)"""
    old = os.environ.pop("RDYHIP_KERNEL", None)
    if kernel:
        os.environ["RDYHIP_KERNEL"] = kernel
    try:
        return [CS.create_operator(c) for c in cases]
    finally:
        os.environ.pop("RDYHIP_KERNEL", None)
        if old is not None:
            os.environ["RDYHIP_KERNEL"] = old


def measure(torch, cases, ens, tiled, cell, rounds):
    B = len(cases)
    mesh = cases[0].mesh
    u = torch.tensor(np.stack([c.u_local for c in cases]), dtype=torch.float64, device="cuda")
    f = torch.zeros((B, mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    fe = torch.zeros_like(f)
    dts = [c.dt for c in cases]

    um, fm = [u[m] for m in range(B)], [f[m] for m in range(B)]      # the members' slices, made once

    def run_ops(ops):
        for m, op in enumerate(ops):
            op.rhs_function(dts[m], um[m], fm[m])
    calls = {"ens": lambda: ens.ensemble_rhs_function(dts, u, fe), "tiled": lambda: run_ops(tiled), "cell": lambda: run_ops(cell)}
    us = {form: [] for form in FORMS}
    for r in range(-1, rounds):                   # round -1: warm-up of every form, not counted
        for form in FORMS:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                calls[form]()
            e1.record()
            torch.cuda.synchronize()
            if r >= 0:
                us[form].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    calls["cell"]()                               # f = the cell operators' F, fe = the ensemble's
    torch.cuda.synchronize()
    a, b = fe.cpu().numpy(), f.cpu().numpy()
    diff = float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))
    return us, diff


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--members", default="2,8,32")
    ap.add_argument("--min-workgroups", type=int, default=1024,
                    help="ENSEMBLE_MIN_WORKGROUPS of the library that is loaded, as stated by the caller (labels the groups column; the library decides)")
    ap.add_argument("--max-per-group", type=int, default=8, help="ENSEMBLE_MAX_PER_GROUP of that library, likewise")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds of each form")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    sizes = [s for s in (SMALL if args.small else SIZES) if not args.only or s[0] in args.only.split(",")]
    counts = [int(b) for b in args.members.split(",")]
    lines = [f"# tools/ensemble_ab.py: min_workgroups {args.min_workgroups}, max_per_group {args.max_per_group}; {args.rounds} interleaved rounds of {LAUNCHES} evaluations of all B members per form; "
             f"device: {torch.cuda.get_device_name(0)}"]
    result = {}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# us per evaluation of all B members, device events, median over the rounds (spread = (max - min) / median)")
    say("# ens = one rdyhip_ensemble_rhs_function; tiled / cell = B rdyhip_rhs_function calls on B operators (default kernel / RDYHIP_KERNEL=cell)")
    say("# groups x per = the member groups of the ensemble launch as computed from the two constants above (stated by the caller, not read from the library)")
    say("# MB = device bytes of the ensemble operator / of the B tiled operators")
    say(f"{'case':<7}{'cells':>9}{'B':>4}{'groups':>9}{'ens us':>10}{'spread':>8}{'tiled us':>10}{'spread':>8}{'cell us':>10}{'spread':>8}"
        f"{'tiled/ens':>10}{'cell/ens':>10}{'ens MB':>9}{'B ops MB':>10}{'F vs cell':>11}")
    for tag, nx, ny in sizes:
        mesh = M.structured_tri_mesh(nx, ny, 1.0, order="tiled")
        blocks = (mesh.num_owned_cells + 255) // 256
        if blocks >= 64:
            blocks = 8 * ((blocks + 7) // 8)                             # dealt to the 8 XCDs in equal chunks
        all_cases = [member_case(CS, mesh, nx, m) for m in range(max(counts))]
        all_tiled, all_cell = operators(CS, all_cases, None), operators(CS, all_cases, "cell")
        for B in counts:
            cases, tiled, cell = all_cases[:B], all_tiled[:B], all_cell[:B]
            ens = operators(CS, cases[:1], "cell")[0]
            ens.enable_ensemble(B)
            for m in range(1, B):
                ens.ensemble_set_mannings_n(m, cases[m].mannings)
            us, diff = measure(torch, cases, ens, tiled, cell, args.rounds)
            m_ = {form: med_spread(us[form]) for form in FORMS}
            g0 = min(B, max(1, (args.min_workgroups + blocks - 1) // blocks))          # the rule of rdyhip_ensemble_enable
            per = min((B + g0 - 1) // g0, args.max_per_group)
            groups = (B + per - 1) // per
            mb_ens = ens.layout_info()["device_bytes"] / 1e6
            mb_ops = sum(o.layout_info()["device_bytes"] for o in tiled) / 1e6
            result[f"{tag}-{B}"] = {"cells": mesh.num_owned_cells, "members": B, "groups": groups, "per_group": per, "f_vs_cell": diff,
                                    "ens_mb": mb_ens, "tiled_ops_mb": mb_ops, **{f"{k}_us": m_[k][0] for k in FORMS},
                                    **{f"{k}_spread": m_[k][1] for k in FORMS}, **{f"{k}_rounds_us": us[k] for k in FORMS}}
            e, t, c = (m_[k][0] for k in FORMS)
            say(f"{tag:<7}{mesh.num_owned_cells:>9}{B:>4}{f'{groups} x {per}':>9}{e:>10.1f}{m_['ens'][1]:>8.3f}{t:>10.1f}{m_['tiled'][1]:>8.3f}"
                f"{c:>10.1f}{m_['cell'][1]:>8.3f}{t / e:>10.2f}{c / e:>10.2f}{mb_ens:>9.1f}{mb_ops:>10.1f}{diff:>11.1e}")
            ens.destroy()
        for o in all_tiled + all_cell:
            o.destroy()
        del all_tiled, all_cell, all_cases
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
