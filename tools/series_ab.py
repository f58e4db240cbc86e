"""A/B of the time series kept on the device: the fused forward-Euler loop (rdyhip_euler_step, F never stored) with a
boundary-flux record and 64 observation sites kept every step, and again every 10 steps, in two forms --

  old    the parent's read path at every record: rdyhip_get_boundary_fluxes per boundary (each a hipDeviceSynchronize and a
         blocking copy), (edge length * flux) / accumulated time in numpy, rdyhip_reset_boundary_fluxes_accum (another
         hipDeviceSynchronize and a hipMemset); the sites' state through a gather on the device and a blocking copy of its
         64 rows (the cheapest way a host has without the new calls; reading the whole state array back would cost more)
  new    rdyhip_series_record for each of the two series (one small launch each, nothing blocks), and ONE rdyhip_series_read of
         each log at the end of the loop, inside the timed window
  none   the loop alone, no series kept (what the other forms add to)

All forms run in ONE process, interleaved round by round (none old new none old new ...), each round timed with device events
around the whole loop of STEPS steps from the same initial state -- the blocking calls of the old form leave the device idle,
and the events see that; median over the rounds and their spread (max - min) / median.  The last round's records of the two
forms are compared: the same 64 bits where finite, NaN at the same places.

Sizes: 0.36 M, 1 M and 10 M triangles (flat-bed dam break, the state of BASELINE.json configs[1]), first order.

usage (GPU box): python tools/series_ab.py [--out FILE] [--rounds R] [--steps K] [--only TAG,TAG] [--small]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("0.36M", 600, 300), ("1M", 1000, 500), ("10M", 2500, 2000)]
SMALL = [("small", 60, 32)]      # rehearsal of the tool itself, not a measurement
FORMS = ("none", "old", "new")
EVERY = (1, 10)
NUM_SITES = 64


def make(nx, ny, capacity):
    """the case, the operator of the old form and the operator of the new form (both series enabled), the sites"""
    from rdycore_amd import cases as CS
    from rdycore_amd import mesh as M
    case = CS.dam_break_case(M.structured_tri_mesh(nx, ny, 1.0, order="tiled"), float(nx), dt=1e-3)
    sites = np.random.default_rng(7).integers(0, case.mesh.num_owned_cells, size=NUM_SITES).astype(np.int32)
    old, new = CS.create_operator(case), CS.create_operator(case)
    new.enable_observation_series(sites, capacity)
    new.enable_boundary_flux_series(capacity)
    return case, old, new, sites


def rounds_of(case, old, new, sites, rounds, steps):
    """`rounds` x EVERY x FORMS, each `steps` steps from the initial state; ({(every, form): [ms per step of each round]},
    {every: same bits})"""
    import torch
    from rdycore_amd.operator import SERIES_BOUNDARY_FLUXES, SERIES_OBSERVATIONS
    mesh = case.mesh
    assert mesh.num_cells == mesh.num_owned_cells       # one rank: every boundary edge is recorded, a site's owned index is its row
    nb, dt = len(mesh.boundaries), case.dt
    lens = [np.asarray(mesh.edge_lengths)[np.asarray(b.edge_ids)][:, None] for b in mesh.boundaries]
    u0 = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    sites_t = torch.as_tensor(sites.astype(np.int64), device="cuda")
    bufs = {form: (u0.clone(), u0.clone()) for form in FORMS}
    ms = {(every, form): [] for every in EVERY for form in FORMS}
    same = {}
    for r in range(-1, rounds):                   # round -1: warm-up of every form (code objects), not counted
        for every in EVERY:
            kept = {}
            for form in FORMS:
                cur, nxt = bufs[form]
                cur.copy_(u0)
                nxt.copy_(u0)
                op = new if form == "new" else old    # (the loop alone runs on the old form's operator: its accumulators are reset below)
                old.reset_boundary_fluxes_accum()
                if new.series_info(SERIES_BOUNDARY_FLUXES)["count"] or new.series_info(SERIES_BOUNDARY_FLUXES)["accumulated_time"]:
                    raise RuntimeError("the new form's log was not left empty")
                flux, obs, T = [], [], 0.0
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for step in range(1, steps + 1):
                    op.euler_step(dt, cur, nxt)
                    cur, nxt = nxt, cur
                    rec = step % every == 0
                    if form == "old":
                        T += dt
                        if rec:
                            obs.append(cur.index_select(0, sites_t).cpu().numpy())
                            acc = [old.boundary_fluxes(b, accumulated=True) for b in range(nb)]
                            with np.errstate(invalid="ignore"):
                                flux.append(np.concatenate([(lens[b] * acc[b]) / T for b in range(nb)]))
                            old.reset_boundary_fluxes_accum()
                            T = 0.0
                    elif form == "new":
                        if rec:
                            new.series_record(SERIES_OBSERVATIONS, step * dt, cur)
                        new.series_add_time(dt)
                        if rec:
                            new.series_record(SERIES_BOUNDARY_FLUXES, step * dt)
                if form == "new":
                    _, fv = new.series_read(SERIES_BOUNDARY_FLUXES)
                    _, ov = new.series_read(SERIES_OBSERVATIONS)
                    new.series_clear(SERIES_BOUNDARY_FLUXES)
                    new.series_clear(SERIES_OBSERVATIONS)
                    flux, obs = fv, ov
                e1.record()
                torch.cuda.synchronize()
                if form == "new" and steps % every:      # a tail of steps without a record: the next loop starts from zeros
                    new.series_record(SERIES_BOUNDARY_FLUXES, 0.0)
                    new.series_clear(SERIES_BOUNDARY_FLUXES)
                if r >= 0:
                    ms[(every, form)].append(e0.elapsed_time(e1) / steps)
                kept[form] = (np.asarray(flux), np.asarray(obs))
            if r == rounds - 1:
                (fa, oa), (fb, ob) = kept["old"], kept["new"]
                nan = np.isnan(fa)
                same[every] = bool(fa.shape == fb.shape and np.array_equal(np.isnan(fb), nan)
                                   and np.array_equal(fa.view(np.int64)[~nan], fb.view(np.int64)[~nan])
                                   and np.array_equal(oa.view(np.int64), ob.view(np.int64)) and fa.shape[0] == steps // every)
    return ms, same


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma-separated case tags")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds of each form")
    if args.steps < max(EVERY):
        raise SystemExit(f"at least {max(EVERY)} steps per round")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("series_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    sizes = [s for s in (SMALL if args.small else SIZES) if not args.only or s[0] in args.only.split(",")]
    lines = [f"# tools/series_ab.py: {args.rounds} interleaved rounds of {args.steps} steps per form; device: {torch.cuda.get_device_name(0)}"]
    result = {}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# ms per forward-Euler step of the whole loop (device events around it), median over the rounds (spread = (max - min) / median)")
    say(f"# a boundary-flux record of every boundary edge and {NUM_SITES} observation sites kept every `every` steps")
    say("# none = the loop alone; old = get_boundary_fluxes per boundary + numpy + reset, sites by gather + copy; new = rdyhip_series_record,")
    say("# one rdyhip_series_read per log at the end (timed); added = what a form costs on top of the loop alone, per step")
    say(f"{'case':<8}{'cells':>10}{'edges':>7}{'every':>7}{'none ms':>10}{'spread':>8}{'old ms':>10}{'spread':>8}{'new ms':>10}{'spread':>8}{'new/old':>9}"
        f"{'added old':>11}{'added new':>11}  same bits")
    for tag, nx, ny in sizes:
        case, old, new, sites = make(nx, ny, args.steps)
        ms, same = rounds_of(case, old, new, sites, args.rounds, args.steps)
        K = sum(b.num_edges for b in case.mesh.boundaries)
        for every in EVERY:
            m = {form: med_spread(ms[(every, form)]) for form in FORMS}
            result[f"{tag}/every{every}"] = {"cells": case.mesh.num_owned_cells, "boundary_edges": K, "same_bits": same[every],
                                             **{f"{k}_ms": m[k][0] for k in FORMS}, **{f"{k}_spread": m[k][1] for k in FORMS}}
            say(f"{tag:<8}{case.mesh.num_owned_cells:>10}{K:>7}{every:>7}{m['none'][0]:>10.4f}{m['none'][1]:>8.3f}{m['old'][0]:>10.4f}{m['old'][1]:>8.3f}"
                f"{m['new'][0]:>10.4f}{m['new'][1]:>8.3f}{m['new'][0] / m['old'][0]:>9.3f}{m['old'][0] - m['none'][0]:>11.4f}{m['new'][0] - m['none'][0]:>11.4f}"
                f"  {same[every]}")
        old.destroy()
        new.destroy()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
