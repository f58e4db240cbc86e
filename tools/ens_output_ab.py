"""A/B of the ensemble output calls (rdyhip_ens_state_planes, rdyhip_ens_error_sums, rdyhip_ens_output_mean_accumulate with all
three variables, rdyhip_ens_stats: one launch each for all B members, two for the sums) against the only alternative a host has
without them: B calls of the per-operator kernels on the members' slices of the same [B, num_cells, 3] array.

  planes   ens: one rdyhip_ens_state_planes (mask 7)        loop: B rdyhip_state_planes (mask 7) into B plane sets
  sums     ens: one rdyhip_ens_error_sums (2 launches)      loop: B rdyhip_error_sums (2 launches and an 80-byte copy each; a real
                                                                  host also needs B blocking _get calls between them, which are
                                                                  not timed: the operator holds one result)
  accum    ens: one rdyhip_ens_output_mean_accumulate of    loop: rdyhip_axpy_owned-shaped launches on B separate accumulators (the
                solution, primitive variables and sources         operator has one accumulator set, so a member loop of
                                                                  rdyhip_output_mean_accumulate does not exist): `B` one axpy per
                                                                  member (72 B/cell, a third of the accumulate's traffic),
                                                                  `3B` one per member and variable (the same traffic)
  stats    ens: one rdyhip_ens_stats (mask 7)               loop: B rdyhip_state_planes (mask 7): what a host must read out to
                                                                  form the statistics itself (the host's work is not timed)

Both sides run in ONE process on the same arrays, interleaved round by round; a round of a form is LAUNCHES calls (of all B members)
between two device events, after a warm-up round of every form.  us per call of all B members = the round / LAUNCHES; median over
the rounds and their spread (max - min) / median.  There is no threshold: the numbers are written down whatever they are.

Workload: 38 448 quads (216 x 178) and 360 000 triangles (600 x 300), B = 8 and 32, random wet states; no reference is read.

usage (GPU box): python tools/ens_output_ab.py [--out FILE] [--rounds R] [--members 8,32] [--small]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("quad-38k", "quad", 216, 178), ("tri-0.36M", "tri", 600, 300)]
SMALL = [("small", "quad", 40, 30)]      # rehearsal of the tool itself, not a measurement
LAUNCHES = 50


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--members", default="8,32")
    ap.add_argument("--small", action="store_true", help="one tiny mesh: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds of each form")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ens_output_ab.py measures on the GPU: no HIP device here")
    torch.cuda.set_device(0)
    from rdycore_amd import _lib
    from rdycore_amd import mesh as M
    from rdycore_amd.operator import Operator, RDyFlowConfig
    lib = _lib.load()
    lines = [f"# tools/ens_output_ab.py: {args.rounds} interleaved rounds of {LAUNCHES} calls of all B members per form; device: {torch.cuda.get_device_name(0)}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# us per call of all B members, device events, median over the rounds (spread = (max - min) / median); loop/ens > 1: the one-launch form is faster")
    say(f"{'mesh':<11}{'cells':>8}{'B':>4}{'call':>8}{'ens us':>10}{'spread':>8}{'loop':>6}{'loop us':>10}{'spread':>8}{'loop/ens':>10}")
    result = {}
    for tag, kind, nx, ny in (SMALL if args.small else SIZES):
        mesh = M.structured_quad_mesh(nx, ny) if kind == "quad" else M.structured_tri_mesh(nx, ny, 1.0, order="tiled")
        no, nc = mesh.num_owned_cells, mesh.num_cells
        assert no == nc
        for B in [int(b) for b in args.members.split(",")]:
            op = Operator.create(RDyFlowConfig(), mesh)
            op.enable_ensemble(B)
            op.ensemble_enable_output_means(7)
            rng = np.random.default_rng(B)
            un = rng.uniform(-1.0, 1.0, (B, nc, 3))
            un[:, :, 0] = 0.5 + np.abs(un[:, :, 0])
            u = torch.tensor(un, dtype=torch.float64, device="cuda")
            um = [u[m] for m in range(B)]                                  # the members' slices, made once
            planes = torch.empty((B, 3, no), dtype=torch.float64, device="cuda")
            pm = [planes[m] for m in range(B)]
            stats = torch.empty((3, 3, no), dtype=torch.float64, device="cuda")
            accs = [torch.zeros((3, nc, 3), dtype=torch.float64, device="cuda") for _ in range(B)]      # B separate accumulator sets
            srcs = torch.tensor(rng.uniform(-1.0, 1.0, (3, no, 3)), dtype=torch.float64, device="cuda")
            dts = np.array([1e-3 * (1.0 + m / 128.0) for m in range(B)])
            h, st = op._h, int(torch.cuda.current_stream().cuda_stream)
            dp = dts.ctypes.data_as(_lib.c_double_p)

            def loop_planes():
                return max(lib.rdyhip_state_planes(h, 7, um[m].data_ptr(), pm[m].data_ptr(), st) for m in range(B))

            def loop_sums():
                return max(lib.rdyhip_error_sums(h, um[m].data_ptr(), None, st) for m in range(B))

            def loop_axpy(nvar):
                def run():
                    return max(lib.rdyhip_axpy_owned(h, dts[m], srcs[v].data_ptr(), accs[m][v].data_ptr(), st) for m in range(B) for v in range(nvar))
                return run
            calls = {
                "planes": (lambda: lib.rdyhip_ens_state_planes(h, 7, u.data_ptr(), planes.data_ptr(), st), {"B": loop_planes}),
                "sums": (lambda: lib.rdyhip_ens_error_sums(h, u.data_ptr(), None, st), {"B": loop_sums}),
                "accum": (lambda: lib.rdyhip_ens_output_mean_accumulate(h, 7, dp, u.data_ptr(), u.data_ptr(), st), {"B": loop_axpy(1), "3B": loop_axpy(3)}),
                "stats": (lambda: lib.rdyhip_ens_stats(h, 7, u.data_ptr(), stats.data_ptr(), st), {"B": loop_planes}),
            }
            for name, (ens, loops) in calls.items():
                forms = {"ens": ens, **loops}
                us = {k: [] for k in forms}
                for r in range(-1, args.rounds):             # round -1: warm-up of every form, not counted
                    for k, fn in forms.items():
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(LAUNCHES):
                            rc = fn()
                            assert not rc, _lib.load().rdyhip_last_error()
                        e1.record()
                        torch.cuda.synchronize()
                        if r >= 0:
                            us[k].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
                e, es = med_spread(us["ens"])
                for k in loops:
                    l, ls = med_spread(us[k])
                    result[f"{tag}-{B}-{name}-{k}"] = {"cells": no, "members": B, "ens_us": e, "ens_spread": es, "loop_us": l, "loop_spread": ls,
                                                       "ens_rounds_us": us["ens"], "loop_rounds_us": us[k]}
                    say(f"{tag:<11}{no:>8}{B:>4}{name:>8}{e:>10.1f}{es:>8.3f}{k:>6}{l:>10.1f}{ls:>8.3f}{l / e:>10.2f}")
            # the results of both sides are in order: the sums of the last member of the loop are those of the ensemble call
            sums = (_lib.RDyHipErrorSums * B)()
            one = _lib.RDyHipErrorSums()
            _lib.check(lib.rdyhip_ens_error_sums_get(h, sums))
            _lib.check(lib.rdyhip_error_sums_get(h, C.byref(one)))
            assert bytes(sums[B - 1]) == bytes(one), "member B - 1: the two forms of the error sums differ"
            assert torch.isfinite(stats).all() and torch.isfinite(planes).all()
            op.destroy()
            del u, um, planes, pm, stats, accs, srcs
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
