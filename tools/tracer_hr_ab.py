"""tracer_hr_kernel beside tracer_rhs_kernel (csrc/tracer_kernels.h) on the same device, mesh and state: ms per
tracers_rhs_function of an operator created with hydrostatic reconstruction (enable_tracers(..., well_balancing=HR)) and of a
plain one, NT = 2, Roe tracer flux, in one process, the two alternating round by round; device events around LAUNCHES
back-to-back evaluations, the median over the rounds and their spread.

What the HR form does more: it reads zc of the cell and of every neighbour (8 more bytes per cell and per neighbour), takes one
more square root per edge (hr_reconstruct) and applies a second wet rule to the own cell.  The two operators evaluate different
schemes, so their F differ by design; the tool only checks that both are finite.  No gate is set on the ratio.

Mesh: a structured triangle mesh in tiled order (default 2500 x 2000 squares = 10 M cells) over a smooth bed, x-y projected; a
lake with a gentle surface slope, so that about a third of the cells is dry and the shore crosses cells of every kind.

usage (GPU box): python tools/tracer_hr_ab.py [--out FILE] [--nx NX --ny NY] [--small]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NT = 2
LAUNCHES = 200      # 0.1 s and more per timed window at 10 M cells
ROUNDS = 7


def bed(x, y):
    return 0.3 * np.sin(0.05 * x) * np.cos(0.04 * y)


def timed(call):
    """ms per evaluation over LAUNCHES back-to-back calls"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--nx", type=int, default=2500)
    ap.add_argument("--ny", type=int, default=2000)
    ap.add_argument("--small", action="store_true", help="60 x 32 squares: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tracer_hr_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    from rdycore_amd import build, codeobj
    from rdycore_amd import mesh as M
    from rdycore_amd.operator import Operator, RDyFlowConfig, WELL_BALANCING_HR, WELL_BALANCING_NONE
    nx, ny = (60, 32) if args.small else (args.nx, args.ny)
    mesh = M.structured_tri_mesh(nx, ny, 1.0, zfunc=bed, order="tiled", project_2d=True)
    nc, no = mesh.num_cells, mesh.num_owned_cells
    c = mesh.cell_centroids
    h = np.maximum(0.0, 0.1 + 0.1 * np.sin(0.013 * c[:, 0]) - mesh.cell_zc)
    u = np.stack([h, 0.1 * h, -0.05 * h, 0.3 * h, 0.05 * h], axis=1)
    dry = float((h == 0.0).mean())
    ud = torch.tensor(u, dtype=torch.float64, device="cuda")
    types = [M.CONDITION_REFLECTING] * len(mesh.boundaries)
    ops = {}
    for tag, wb in (("plain", WELL_BALANCING_NONE), ("hr", WELL_BALANCING_HR)):
        op = Operator.create(RDyFlowConfig(well_balancing=wb), mesh, types)
        op.set_domain_mannings_n(np.full(no, 0.03))
        op.enable_tracers(NT, well_balancing=wb)
        ops[tag] = op
    f = torch.empty((no, 3 + NT), dtype=torch.float64, device="cuda")
    dt = 1e-3
    calls = {tag: (lambda op=op: op.tracers_rhs_function(dt, ud, f)) for tag, op in ops.items()}
    for tag, call in calls.items():          # warm-up: code objects loaded, every array touched; and both results are finite
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(f).all()), tag
    times = {tag: [] for tag in calls}
    for _ in range(ROUNDS):                  # alternating: a drift of the device or the host hits both alike
        for tag, call in calls.items():
            times[tag].append(timed(call))
    regs = {}
    for k, v in codeobj.kernel_resources(build.lib_path()).items():
        for tag, name in (("plain", f"tracer_rhs_kernel<3, {NT}, false>"), ("hr", f"tracer_hr_kernel<3, {NT}, false>")):
            if name in k:
                regs[tag] = v["vgpr"] + v["agpr"]
    med = {tag: statistics.median(v) for tag, v in times.items()}
    lines = [f"# tools/tracer_hr_ab.py: ms per tracers_rhs_function, NT = {NT}, Roe; device events around {LAUNCHES} back-to-back evaluations, "
             f"{ROUNDS} rounds alternating plain / hr; device: {torch.cuda.get_device_name(0)}",
             f"# mesh: {nx} x {ny} squares, {nc} triangles (tiled order, x-y projected), {100 * dry:.1f} % of the cells dry",
             f"{'form':<8}{'median ms':>12}{'min':>10}{'max':>10}{'GB/s of state':>16}{'VGPRs':>8}"]
    for tag in ("plain", "hr"):
        v = times[tag]
        # the least traffic of one evaluation: the own row read, F written (the neighbours' rows mostly hit the caches)
        gbs = 2 * 8 * (3 + NT) * no / (med[tag] * 1e-3) / 1e9
        lines.append(f"{tag:<8}{med[tag]:>12.4f}{min(v):>10.4f}{max(v):>10.4f}{gbs:>16.1f}{regs.get(tag, -1):>8}")
    lines.append(f"ratio hr / plain (medians): {med['hr'] / med['plain']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    for op in ops.values():
        op.destroy()


if __name__ == "__main__":
    main()
