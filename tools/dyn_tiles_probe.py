"""When the persistent workgroups of the first-order tiled kernel start and finish (profiles/dyn_tiles_wg_times.json).

Needs a PROBE build of the library (tools/probes/wg_times.patch applied to a copy of rdycore_amd/csrc, built like
rdycore_amd/build.py builds the real one): thread 0 of every workgroup stores wall_clock64() (100 MHz) at entry and after its
last tile, rdyhip_probe_wg_times() copies the [grid][2] table out.  The patch never goes into the library proper.
(Since the tile loop takes its addresses from scalar bases the patch also puts a readfirstlane of both halves of the base into
lane_ptr, with unsigned casts: with the entry store in place hipcc cannot prove the bases uniform in the kernels without the
dynamic walk and would refuse to compile them.  The headline kernel of such a build is the product's instruction stream plus
the two stores.  That form of the patch applies and compiles; it has not been run on a GPU yet, RESULTS_LOG section 27.)

    RDYHIP_LIB=/path/to/probe.so python tools/dyn_tiles_probe.py --walks static,dynamic --out wg_times.json [--label L]

One warm launch of bench.py's c3 and c2 workloads per walk (RDYHIP_TILE_WALK is read at create).  Block ids are dealt round-robin
to the XCDs: blockIdx.x & 7 is the XCD.  Per XCD and overall: the earliest start, mean / median / p95 / max of the end times
(microseconds after the launch's earliest start) and tail = 1 - mean(end - t0) / max(end - t0); whether the workgroups' spread
is inside the XCDs or between them."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TICK_US = 0.01  # wall_clock64: 100 MHz


def stats(start, end, t0):
    e = (end - t0) * TICK_US
    return {"workgroups": int(e.size), "earliest_start_us": round(float((start.min() - t0) * TICK_US), 2),
            "latest_start_us": round(float((start.max() - t0) * TICK_US), 2),
            "end_mean_us": round(float(e.mean()), 2), "end_median_us": round(float(np.median(e)), 2),
            "end_p95_us": round(float(np.percentile(e, 95)), 2), "end_min_us": round(float(e.min()), 2), "end_max_us": round(float(e.max()), 2),
            "tail": round(float(1.0 - e.mean() / e.max()), 4)}


def measure(lib, op, case, u, f, torch, warm=30, launches=5):
    grid = op.layout_info()["persistent_grid"]
    out = []
    for _ in range(warm):
        op.rhs_function(case.dt, u, f)
    torch.cuda.synchronize()
    for _ in range(launches):   # each launch alone: the table is the last launch's
        op.rhs_function(case.dt, u, f)
        torch.cuda.synchronize()
        t = np.zeros((grid, 2), dtype=np.uint64)
        rc = lib.rdyhip_probe_wg_times(t.ctypes.data_as(C.c_void_p), C.c_int(grid))
        assert rc == 0, rc
        t = t.astype(np.int64)
        start, end = t[:, 0], t[:, 1]
        assert (end >= start).all() and start.min() > 0
        t0 = start.min()
        x = np.arange(grid) & 7
        per = [stats(start[x == k], end[x == k], t0) for k in range(8)]
        allw = stats(start, end, t0)
        xm = np.array([p["end_mean_us"] for p in per])
        within = float(np.mean([((end[x == k] - t0) * TICK_US).std() for k in range(8)]))
        out.append({"all": allw, "per_xcd": per, "between_xcd_spread_of_mean_end_us": round(float(xm.max() - xm.min()), 2),
                    "within_xcd_std_of_end_us_mean": round(within, 2),
                    "spread_is_mostly": "between XCDs" if xm.max() - xm.min() > 2.0 * within else "within XCDs"})
    out.sort(key=lambda r: r["all"]["end_max_us"])
    med = out[len(out) // 2]   # the launch with the median duration
    med["launches_measured"] = launches
    med["end_max_us_of_each_launch"] = [r["all"]["end_max_us"] for r in out]
    med["tail_of_each_launch"] = [r["all"]["tail"] for r in out]
    return med


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walks", default="static")
    p.add_argument("--out", required=True)
    p.add_argument("--label", default="")
    p.add_argument("--workloads", default="c3,c2")
    a = p.parse_args()
    import torch
    from rdycore_amd import _lib, build
    from rdycore_amd import cases as CS
    lib = _lib.load()
    raw = C.CDLL(build.lib_path())
    if not hasattr(raw, "rdyhip_probe_wg_times"):
        raise SystemExit("RDYHIP_LIB is not a probe build (tools/probes/wg_times.patch)")
    res = {"library": os.path.basename(build.lib_path()), "label": a.label, "unit": "microseconds after the launch's earliest workgroup start",
           "clock": "wall_clock64, 100 MHz"}
    if os.path.exists(a.out):
        prev = json.load(open(a.out))
    else:
        prev = {}
    for wl in a.workloads.split(","):
        args = bench.parse(["--workload", wl])
        case = bench.build_case(args, 0, 1)
        u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda:0")
        f = torch.empty((case.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda:0")
        for walk in a.walks.split(","):
            os.environ["RDYHIP_TILE_WALK"] = walk
            op = CS.create_operator(case)
            info = op.layout_info()
            r = measure(raw, op, case, u, f, torch)
            r["num_tiles"], r["persistent_grid"] = info["num_tiles"], info["persistent_grid"]
            res[f"{wl}_{walk}"] = r
            print(wl, walk, json.dumps(r["all"]), r["spread_is_mostly"], r["between_xcd_spread_of_mean_end_us"], r["within_xcd_std_of_end_us_mean"], flush=True)
            op.destroy()
        del u, f, case
    prev[a.label or res["library"]] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(prev, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
