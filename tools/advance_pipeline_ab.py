"""The RDyAdvance-shaped loop of tools/advance_pattern.py (--refresh setter) with the Courant read-back taken three ways, in one
process, alternating, on the c3 workload:

    blocking    set source; steps; rdyhip_update_diagnostics + get           (the sequence before the non-blocking read-back)
    pipelined   set source; rdyhip_diagnostics_wait + get (if a read is out); steps; rdyhip_diagnostics_begin
    fixed       set source; steps                                            (fixed dt: nothing in an interval synchronises)

per coupling interval, followed by `gap` ms of host work (a busy wait).  Every sample is `--intervals` intervals; the figure is
the wall time from the first interval's start to the moment the last result is on the host (blocking: its last update;
pipelined: a final wait; fixed: a device synchronise), gaps included, per step.  The steps run with dt = 0: the state stays
put and every interval does the same work.  The rain is a host array of one value per owned cell, uniform or a ramp (a ramp is
really uploaded; a uniform array is recognised by the setter, uniform_fields.h).

For every configuration the one condition is printed: the pipelined median must not exceed the blocking median by more than
the spread (max - min) of the blocking samples.  What remains between pipelined and fixed is the device restarting from idle
every interval (dt needs the last step's Courant number), which the read-back cannot remove.

usage (GPU box): python tools/advance_pipeline_ab.py > profiles/advance_pipeline_ab.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="c3")
ap.add_argument("--intervals", type=int, default=12)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps-per-interval", default="20,100")
ap.add_argument("--gaps-ms", default="0,2,10")
ap.add_argument("--rain", default="uniform,ramp")
a = ap.parse_args()

args = bench.parse(["--no-cpu-baseline", "--workload", a.workload])
torch.cuda.set_device(0)
from rdycore_amd import cases as CS

case = bench.build_case(args, 0, 1)
op = CS.create_operator(case)
n_owned = case.mesh.num_owned_cells
u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
u2 = torch.empty_like(u)
RAIN = {"uniform": np.full(n_owned, 1e-5), "ramp": 1e-5 * (1.0 + np.arange(n_owned) / n_owned)}
LEGS = ("blocking", "pipelined", "fixed")


def busy_wait(ms):
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        pass


def sample(leg, rain, nsteps, gap_ms, intervals):
    """wall seconds of `intervals` intervals of one leg"""
    torch.cuda.synchronize()
    out = False
    courant = -1.0
    t0 = time.perf_counter()
    for _ in range(intervals):
        op.set_domain_external_source(0, rain, ordered=True)
        if out:
            op.diagnostics_wait()
            courant = op.get_diagnostics().max_courant_num
            out = False
        cur, nxt = u, u2
        for _ in range(nsteps):
            op.euler_step(0.0, cur, nxt)
            cur, nxt = nxt, cur
        if leg == "blocking":
            op.update_diagnostics()
            courant = op.get_diagnostics().max_courant_num
        elif leg == "pipelined":
            op.diagnostics_begin()
            out = True
        busy_wait(gap_ms)
    if out:
        op.diagnostics_wait()
        courant = op.get_diagnostics().max_courant_num
    torch.cuda.synchronize()
    assert leg == "fixed" or courant >= 0.0
    return time.perf_counter() - t0


print(f"workload {a.workload}: {n_owned} owned cells, {a.intervals} intervals per sample, {a.rounds} rounds, legs alternating; ms per step (wall, gaps included)")
for leg in LEGS:                                    # conditioning: allocations, first launches, the pinned record of the first begin
    sample(leg, RAIN["ramp"], 20, 0.0, 2)
failed = []
for rain_name in a.rain.split(","):
    for nsteps in map(int, a.steps_per_interval.split(",")):
        for gap in map(float, a.gaps_ms.split(",")):
            ms = {leg: [] for leg in LEGS}
            for _ in range(a.rounds):
                for leg in LEGS:
                    ms[leg].append(sample(leg, RAIN[rain_name], nsteps, gap, a.intervals) / (a.intervals * nsteps) * 1e3)
            med = {leg: statistics.median(ms[leg]) for leg in LEGS}
            spread = max(ms["blocking"]) - min(ms["blocking"])
            ok = med["pipelined"] <= med["blocking"] + spread
            gap_left = (med["pipelined"] - med["fixed"]) / (med["blocking"] - med["fixed"]) if med["blocking"] > med["fixed"] else float("nan")
            print(f"\nrain {rain_name}, {nsteps} steps per interval, host gap {gap:g} ms")
            for leg in LEGS:
                print(f"  {leg:9s} median {med[leg]:.4f}  samples " + " ".join(f"{x:.4f}" for x in ms[leg]))
            print(f"  pipelined / blocking {med['pipelined'] / med['blocking']:.3f}, pipelined / fixed {med['pipelined'] / med['fixed']:.3f}, "
                  f"blocking / fixed {med['blocking'] / med['fixed']:.3f}; of the blocking leg's gap to fixed dt {gap_left:.2f} remains")
            print(f"  condition (pipelined median <= blocking median + blocking spread {spread:.4f}): {'holds' if ok else 'FAILS'}")
            sys.stdout.flush()
            if not ok:
                failed.append((rain_name, nsteps, gap))
print(f"\nconfigurations in which the condition fails: {failed if failed else 'none'}")
op.destroy()
