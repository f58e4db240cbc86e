"""A/B of one ensemble evaluation under hydrostatic reconstruction against the only way to evaluate B such members without it: B
operators created with hydrostatic reconstruction on the same mesh and B back-to-back rdyhip_rhs_function calls, one per member.

  ens     one rdyhip_ensemble_rhs_function on one HR operator with B members (rdyhip_ens_hr_enable: ensemble_hr_kernel, one launch)
  tiled   B rdyhip_rhs_function calls on B HR operators, the default tiled HR kernel (there is no cell-centric HR kernel)

Both forms run in ONE process on the same member states, interleaved round by round (ens tiled ens tiled ...); a round of a form is
LAUNCHES evaluations of all B members between two device events, after a warm-up round of either form.  us per evaluation of all B
members = the round / LAUNCHES; median over the rounds and their spread (max - min) / median.  The F of the ensemble launch is
compared with the tiled operators' (largest relative difference: the two kernels add a cell's edges in different orders).  Beside
the times: the device bytes of the one ensemble operator against those of the B operators, and the member groups the launch ran
with.  There is no threshold: the numbers are written down whatever they are.

Workload: a structured triangle mesh in tiled order over a smooth bed, x-y projected, at 0.36 M and 1 M triangles; member m is a
lake with a gentle surface slope whose level rises with m (about a third of the cells dry in member 0, the shore crosses cells of
every kind), Manning's n 0.03 (1 + m / 32), dt = 1e-3 (1 + m / 128); B = 2, 8, 32.  The B operators of the baseline are created
once per size, for the largest B, and the smaller counts use the first B of them.

The group rule (ENSEMBLE_MIN_WORKGROUPS = 1024, ENSEMBLE_MAX_PER_GROUP = 8 in csrc/ensemble_kernels.h) was measured on the plain
family and is kept as it is; the `groups` column is computed here from the same two numbers.

usage (GPU box): python tools/ensemble_hr_ab.py [--out FILE] [--rounds R] [--only TAG,TAG] [--members 2,8,32] [--small]"""
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
FORMS = ("ens", "tiled")
LAUNCHES = 50
MIN_WORKGROUPS, MAX_PER_GROUP = 1024, 8


def bed(x, y):
    return 0.3 * np.sin(0.05 * x) * np.cos(0.04 * y)


def member_state(mesh, m):
    c = mesh.cell_centroids
    h = np.maximum(0.0, 0.1 + 0.004 * m + 0.1 * np.sin(0.013 * c[:, 0]) - mesh.cell_zc)
    return np.stack([h, 0.1 * h, -0.05 * h], axis=1)


def measure(torch, states, dts, ens, tiled, rounds):
    B = len(tiled)
    no = ens.mesh.num_owned_cells
    u = torch.tensor(np.stack(states), dtype=torch.float64, device="cuda")
    f = torch.zeros((B, no, 3), dtype=torch.float64, device="cuda")
    fe = torch.zeros_like(f)
    um, fm = [u[m] for m in range(B)], [f[m] for m in range(B)]      # the members' slices, made once

    def run_ops():
        for m, op in enumerate(tiled):
            op.rhs_function(dts[m], um[m], fm[m])
    calls = {"ens": lambda: ens.ensemble_rhs_function(dts, u, fe), "tiled": run_ops}
    us = {form: [] for form in FORMS}
    for r in range(-1, rounds):                   # round -1: warm-up of either form, not counted
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
    a, b = fe.cpu().numpy(), f.cpu().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return us, float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--members", default="2,8,32")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds of each form")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_hr_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    os.environ.pop("RDYHIP_KERNEL", None)         # an HR operator exists in the tiled form only
    from rdycore_amd import build, codeobj
    from rdycore_amd import mesh as M
    from rdycore_amd.operator import Operator, RDyFlowConfig, WELL_BALANCING_HR
    sizes = [s for s in (SMALL if args.small else SIZES) if not args.only or s[0] in args.only.split(",")]
    counts = [int(b) for b in args.members.split(",")]
    regs = sorted(v["vgpr"] + v["agpr"] for k, v in codeobj.kernel_resources(build.lib_path()).items() if "ensemble_hr_kernel<3, 0, false>" in k)
    lines = [f"# tools/ensemble_hr_ab.py: min_workgroups {MIN_WORKGROUPS}, max_per_group {MAX_PER_GROUP} (the plain family's rule, kept); {args.rounds} interleaved rounds of "
             f"{LAUNCHES} evaluations of all B members per form; ensemble_hr_kernel<3, 0, false>: {regs} VGPRs; device: {torch.cuda.get_device_name(0)}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# us per evaluation of all B members, device events, median over the rounds (spread = (max - min) / median)")
    say("# ens = one rdyhip_ensemble_rhs_function after rdyhip_ens_hr_enable; tiled = B rdyhip_rhs_function calls on B HR operators (default tiled HR kernel)")
    say("# MB = device bytes of the ensemble operator / of the B tiled operators; dry = share of dry cells in member 0 .. member B - 1")
    say(f"{'case':<7}{'cells':>9}{'B':>4}{'groups':>9}{'ens us':>10}{'spread':>8}{'tiled us':>10}{'spread':>8}{'tiled/ens':>10}{'ens MB':>9}{'B ops MB':>10}"
        f"{'F vs tiled':>12}{'dry':>14}")
    result = {}
    for tag, nx, ny in sizes:
        mesh = M.structured_tri_mesh(nx, ny, 1.0, zfunc=bed, order="tiled", project_2d=True)
        no = mesh.num_owned_cells
        blocks = (no + 255) // 256
        if blocks >= 64:
            blocks = 8 * ((blocks + 7) // 8)                             # dealt to the 8 XCDs in equal chunks
        types = [M.CONDITION_REFLECTING] * len(mesh.boundaries)
        cfg = RDyFlowConfig(well_balancing=WELL_BALANCING_HR)
        nmax = max(counts)
        states = [member_state(mesh, m) for m in range(nmax)]
        manns = [np.full(no, 0.03 * (1.0 + m / 32.0)) for m in range(nmax)]
        dts = [1e-3 * (1.0 + m / 128.0) for m in range(nmax)]
        all_tiled = []
        print(f"# {tag}: {no} cells, creating {nmax} operators", file=sys.stderr, flush=True)
        for m in range(nmax):
            op = Operator.create(cfg, mesh, types)
            op.set_domain_mannings_n(manns[m])
            all_tiled.append(op)
        for B in counts:
            ens = Operator.create(cfg, mesh, types)
            ens.set_domain_mannings_n(manns[0])
            ens.enable_ensemble(B, well_balancing=WELL_BALANCING_HR)
            for m in range(1, B):
                ens.ensemble_set_mannings_n(m, manns[m])
            us, diff = measure(torch, states[:B], dts[:B], ens, all_tiled[:B], args.rounds)
            m_ = {form: med_spread(us[form]) for form in FORMS}
            g0 = min(B, max(1, (MIN_WORKGROUPS + blocks - 1) // blocks))          # the rule of rdyhip_ensemble_enable
            per = min((B + g0 - 1) // g0, MAX_PER_GROUP)
            groups = (B + per - 1) // per
            mb_ens = ens.layout_info()["device_bytes"] / 1e6
            mb_ops = sum(o.layout_info()["device_bytes"] for o in all_tiled[:B]) / 1e6
            dry = [float((states[m][:, 0] == 0.0).mean()) for m in (0, B - 1)]
            result[f"{tag}-{B}"] = {"cells": no, "members": B, "groups": groups, "per_group": per, "f_vs_tiled": diff, "ens_mb": mb_ens, "tiled_ops_mb": mb_ops,
                                    **{f"{k}_us": m_[k][0] for k in FORMS}, **{f"{k}_spread": m_[k][1] for k in FORMS},
                                    **{f"{k}_rounds_us": us[k] for k in FORMS}}
            e, t = (m_[k][0] for k in FORMS)
            say(f"{tag:<7}{no:>9}{B:>4}{f'{groups} x {per}':>9}{e:>10.1f}{m_['ens'][1]:>8.3f}{t:>10.1f}{m_['tiled'][1]:>8.3f}{t / e:>10.2f}{mb_ens:>9.1f}{mb_ops:>10.1f}"
                f"{diff:>12.1e}{f'{dry[0]:.2f} .. {dry[1]:.2f}':>14}")
            ens.destroy()
        for o in all_tiled:
            o.destroy()
        del all_tiled, states
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
