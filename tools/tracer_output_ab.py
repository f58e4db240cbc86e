"""The tracer output kernels (csrc/tracer_output_kernels.h) beside axpy_owned_kernel on the same device: us per launch with
device events around LAUNCHES back-to-back launches, for NT = 2 and 7 (rows of N = 5 and 10 doubles), each next to the ratio
of the bytes it moves per cell to axpy_owned_kernel's 72 --

  planes       tracer_planes_kernel, conserved and primitive form, k = 1 and k = N planes       (8 N + 8 k) / 72
  accumulate   tracer_output_accumulate_kernel, one variable (the solution) and all three       24 N / 72 per variable
               (solution and primitive variables from one array: its rows are read once, so      (three: (8 N + 3 * 16 N) / 72)
               three variables move 8 N less than three times one)
  sums         tracer_error_partial_kernel + tracer_error_finalize_kernel + the copy of          (8 N [+ 8 N exact] + 8) / 72
               3 N + 1 doubles, without and with an exact solution

No gate is set on these numbers; they are written down whatever they are.  Sizes: 0.36 M, 1 M and 10 M triangles (flat-bed
dam break, the meshes of tools/readout_ab.py), the tracer columns a fixed fraction of h.

usage (GPU box): python tools/tracer_output_ab.py [--out FILE] [--only TAG,TAG] [--small]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("0.36M", 600, 300), ("1M", 1000, 500), ("10M", 2500, 2000)]
SMALL = [("small", 60, 32)]      # rehearsal of the tool itself, not a measurement
NTS = (2, 7)
LAUNCHES = 50


def timed(call):
    """us per launch"""
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES


def kernel_times(case, nt):
    """{name: (us per launch, bytes per cell)} for one mesh and tracer count"""
    import torch
    from rdycore_amd import _lib
    from rdycore_amd import cases as CS
    from rdycore_amd.operator import OUTPUT_SOLUTION, TRACER_FORM_CONSERVED, TRACER_FORM_PRIMITIVE, _ptr, _stream
    mesh, n = case.mesh, 3 + nt
    no = mesh.num_owned_cells
    op = CS.create_operator(case)
    op.enable_tracers(nt)
    lib = _lib.load()
    u3 = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f3 = torch.zeros((no, 3), dtype=torch.float64, device="cuda")
    u = torch.cat([u3] + [u3[:, :1] * (0.1 * (j + 1)) for j in range(nt)], dim=1).contiguous()
    exact = u[torch.as_tensor(np.asarray(mesh.cell_owned_to_local), device="cuda")].contiguous()
    out = torch.empty((n, no), dtype=torch.float64, device="cuda")
    full = (1 << n) - 1
    op.tracers_enable_output_means(7)
    op.tracers_error_sums(u)                 # first use: the areas and records are allocated
    res = {"axpy": (timed(lambda: op.axpy_owned(0.0, f3, u3)), 72)}
    for form, tag in ((TRACER_FORM_CONSERVED, "cons"), (TRACER_FORM_PRIMITIVE, "prim")):
        res[f"planes {tag} k=1"] = (timed(lambda: op.tracers_state_planes(u, 8, form, out=out)), 8 * n + 8)
        res[f"planes {tag} k=N"] = (timed(lambda: op.tracers_state_planes(u, full, form, out=out)), 16 * n)
    res["accumulate 1 var"] = (timed(lambda: op.tracers_accumulate_output_means(OUTPUT_SOLUTION, 0.0, u, None)), 24 * n)
    res["accumulate 3 vars"] = (timed(lambda: op.tracers_accumulate_output_means(7, 0.0, u, u)), 8 * n + 3 * 16 * n)
    # the error sums: enqueue through the C ABI without reading any result
    res["sums"] = (timed(lambda: _lib.check(lib.rdyhip_tracer_error_sums(op._h, _ptr(u), None, _stream()))), 8 * n + 8)
    res["sums exact"] = (timed(lambda: _lib.check(lib.rdyhip_tracer_error_sums(op._h, _ptr(u), _ptr(exact), _stream()))), 16 * n + 8)
    op.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tracer_output_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    sizes = [s for s in (SMALL if args.small else SIZES) if not args.only or s[0] in args.only.split(",")]
    lines = [f"# tools/tracer_output_ab.py: us per launch, device events around {LAUNCHES} back-to-back launches; device: {torch.cuda.get_device_name(0)}"]
    result = {}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# x axpy = the kernel's time / axpy_owned_kernel's on the same mesh; bytes = its bytes per cell / axpy's 72; over = x axpy / bytes")
    say(f"{'case':<8}{'NT':>4}  {'kernel':<20}{'us':>10}{'x axpy':>9}{'bytes':>9}{'over':>8}")
    for tag, nx, ny in sizes:
        case = CS.dam_break_case(M.structured_tri_mesh(nx, ny, 1.0, order="tiled"), float(nx), dt=1e-3)
        for nt in NTS:
            res = kernel_times(case, nt)
            axpy = res["axpy"][0]
            for name, (us, nbytes) in res.items():
                say(f"{tag:<8}{nt:>4}  {name:<20}{us:>10.1f}{us / axpy:>9.3f}{nbytes / 72:>9.3f}{(us / axpy) / (nbytes / 72):>8.2f}")
            result[f"{tag} NT={nt}"] = {"cells": case.mesh.num_owned_cells, **{k: {"us": v[0], "bytes_per_cell": v[1]} for k, v in res.items()}}
        del case
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
