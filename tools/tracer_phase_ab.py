"""A/B of rdyhip_tracers_rhs_function between two builds of the library (the recipe of profiles/RESULTS_LOG.md section 22): does
the phase test in tracer_rhs_kernel cost the unphased call anything?

  one sample     200 back-to-back launches after 20 warm-up launches, device events around the 200, ms per launch
  one series     seven samples in ONE fresh process that loads one library through RDYHIP_LIB
  the A/B        the two libraries alternate, process by process, on the same box in one call: A B A B ... `--rounds` times;
                 reported per library: every series, its median, and the spread (min .. max) of each series without its first
                 sample (the first use of the kernel in the process is the slowest)

Case: 1 000 x 500 x 2 = 1 000 000-cell structured_tri_mesh, tiled cell order, MMS-style state over sinusoidal bathymetry,
Manning field, rain source, a dry disc, Dirichlet + reflecting boundaries, NT = 2, Roe tracer flux.

usage (GPU box): python tools/tracer_phase_ab.py --a PARENT.so --b THIS.so [--rounds 2] [--out profiles/tracer_phase_ab.txt] [--small]
                 python tools/tracer_phase_ab.py --series            (one series of the library RDYHIP_LIB names; prints one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAUNCHES, WARMUP, SAMPLES, NT = 200, 20, 7, 2


def series(small):
    import numpy as np
    import torch
    from rdycore_amd import build, codeobj
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    nx, ny = (100, 50) if small else (1000, 500)
    K = 2 * np.pi / 200.0
    mesh = M.structured_tri_mesh(nx, ny, 1.0, zfunc=CS.mms_bathymetry(K=K), order="tiled")
    case = CS.friction_slope_case(mesh, float(nx), float(ny), dt=1e-3, K=K)
    case.condition_types = [M.CONDITION_REFLECTING if t == M.CONDITION_CRITICAL_OUTFLOW else t for t in case.condition_types]
    op = CS.create_operator(case)
    op.enable_tracers(NT, 0)
    rng = np.random.default_rng(22)
    no = mesh.num_owned_cells
    for j in range(NT):
        op.tracers_set_source(j, rng.normal(size=no) * 1e-3)
    for b, vals in case.boundary_values.items():
        op.tracers_set_boundary_values(b, np.concatenate([vals, vals[:, :1] * rng.uniform(0.0, 0.8, (vals.shape[0], NT))], axis=1))
    u = torch.tensor(np.concatenate([case.u_local, case.u_local[:, :1] * rng.uniform(0.0, 0.8, (mesh.num_cells, NT))], axis=1),
                     dtype=torch.float64, device="cuda")
    f = torch.empty((no, 3 + NT), dtype=torch.float64, device="cuda")
    ms = []
    for _ in range(SAMPLES):
        for _ in range(WARMUP):
            op.tracers_rhs_function(case.dt, u, f)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            op.tracers_rhs_function(case.dt, u, f)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / LAUNCHES)
    lib = build.lib_path()
    name = next(k for k in codeobj.kernel_resources(lib) if "tracer_rhs_kernel<3, 2, false>" in k)
    res = codeobj.kernel_resources(lib)[name]
    code = codeobj.kernel_bytes(lib)                                   # by mangled name
    size = next(len(b) for m, b in code.items() if "tracer_rhs_kernel" in m and "ILi3ELi2ELb0E" in m)
    print(json.dumps({"lib": lib, "cells": no, "ms": ms, "f_sum": float(f.sum().item()), "vgpr": res["vgpr"], "sgpr": res["sgpr"],
                      "code_bytes": size, "code_sha": codeobj.kernel_sha(lib, name)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", action="store_true")
    ap.add_argument("--small", action="store_true", help="a rehearsal of the tool on 10 000 cells, not a measurement")
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_phase_ab.txt"))
    args = ap.parse_args()
    if args.series:
        return series(args.small)
    runs = {"A": [], "B": []}
    for r in range(args.rounds):
        for tag, lib in (("A", args.a), ("B", args.b)):
            env = dict(os.environ, RDYHIP_LIB=os.path.abspath(lib), RDYHIP_KERNEL="cell")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--series"] + (["--small"] if args.small else []), env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode:
                sys.exit(f"the series of {lib} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            out = p.stdout
            runs[tag].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
    lines = [f"rdyhip_tracers_rhs_function, tracer_rhs_kernel<3, 2, false>, {runs['A'][0]['cells']} cells, NT = {NT}: ms per launch,",
             f"{LAUNCHES} launches after {WARMUP} warm-ups, {SAMPLES} samples per process, processes alternating A B A B (A = the parent commit's library, B = this build)"]
    for tag in ("A", "B"):
        for i, r in enumerate(runs[tag]):
            rest = r["ms"][1:]
            lines.append(f"{tag} process {i}: " + " ".join(f"{x:.5f}" for x in r["ms"]) + f" | median {statistics.median(r['ms']):.5f} | without the first: "
                         f"{min(rest):.5f} .. {max(rest):.5f}")
        r = runs[tag][0]
        lines.append(f"{tag} kernel: {r['vgpr']} VGPR, {r['sgpr']} SGPR, {r['code_bytes']} bytes of code, sha {r['code_sha'][:16]}, sum(F) = {r['f_sum']!r}")
    a_rest = [x for r in runs["A"] for x in r["ms"][1:]]
    meds = [statistics.median(r["ms"]) for r in runs["B"]]
    lines.append(f"A's spread over its samples without the first of each process: {min(a_rest):.5f} .. {max(a_rest):.5f}; B's medians: " +
                 " ".join(f"{m:.5f}" for m in meds) + (" -- inside" if all(min(a_rest) <= m <= max(a_rest) for m in meds) else " -- OUTSIDE"))
    lines.append("same F: " + str(all(r["f_sum"] == runs["A"][0]["f_sum"] for t in runs for r in runs[t])))
    text = "\n".join(lines) + "\n"
    print(text)
    if not args.small:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
