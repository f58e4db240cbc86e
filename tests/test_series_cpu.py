"""CPU: the time series kept on the device (rdyhip_series_*, csrc/series_kernels.h, csrc/series_plan.h) as far as they go
without one -- the symbols and their argument errors, the record plan of the boundary-flux series against a numpy restatement
of the reference's loops (src/time_series.c:270-335) and, as a stand-alone program, under the address and undefined-behaviour
sanitizers (tests/host/series_plan_dump.cpp; never loaded into Python, never run on a device), the two kernels in the code
object, and which calls EulerStepper(series=...) makes around a stand-in operator that records them."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from rdycore_amd import _lib, build
from rdycore_amd import operator as O
from rdycore_amd.operator import RDyFlowConfig, plan_series_boundary_edges
from rdycore_amd.timestep import EulerStepper, TimeSeries

from test_gpu_output_mean import MESHES, _mesh
from test_layout_tables_cpu import FLAGS, write_case
from test_output_mean_cpu import RecordingOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "series_plan_dump.cpp")
NEW_SYMBOLS = ["rdyhip_series_observations_enable", "rdyhip_series_boundary_fluxes_enable", "rdyhip_series_boundary_edges",
               "rdyhip_series_plan_boundary_edges", "rdyhip_series_boundary_fluxes_add_time", "rdyhip_series_record", "rdyhip_series_info",
               "rdyhip_series_read", "rdyhip_series_device_log", "rdyhip_series_clear"]


# ---- symbols and argument errors -----------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert (O.SERIES_OBSERVATIONS, O.SERIES_BOUNDARY_FLUXES) == (1, 2)
    assert lib.rdyhip_version() == 110


def test_argument_errors_without_a_device():
    lib = _lib.load()
    n, t, p = C.c_int32(), C.c_double(), C.c_void_p()
    e, b = _lib.c_int32_p(), _lib.c_int32_p()
    ids = (C.c_int32 * 2)(0, 1)
    calls = [lambda: lib.rdyhip_series_observations_enable(None, 2, ids, 4),
             lambda: lib.rdyhip_series_boundary_fluxes_enable(None, 0, None, 4),
             lambda: lib.rdyhip_series_boundary_edges(None, C.byref(n), C.byref(e), C.byref(b)),
             lambda: lib.rdyhip_series_boundary_fluxes_add_time(None, 0.1),
             lambda: lib.rdyhip_series_record(None, 1, 0.0, None, None),
             lambda: lib.rdyhip_series_record(None, 2, 0.0, None, None),
             lambda: lib.rdyhip_series_info(None, 1, C.byref(n), C.byref(n), C.byref(n), C.byref(t)),
             lambda: lib.rdyhip_series_read(None, 2, 0, 0, None, None, None),
             lambda: lib.rdyhip_series_device_log(None, 1, C.byref(p)),
             lambda: lib.rdyhip_series_clear(None, 2),
             lambda: lib.rdyhip_series_plan_boundary_edges(None, 0, None, 0, None, C.byref(n), None, None)]
    for call in calls:
        # PETSC_ERR_USER = 83, reported before any HIP call
        assert call() == 83
        assert b"null" in lib.rdyhip_last_error()


# ---- the record plan -----------------------------------------------------------------------------------------------------------

def numpy_plan(mesh, listed):
    """RecordBoundaryFluxes / WriteBoundaryFluxes: boundaries in ascending index, the listed ones only; a boundary's edges in
    edge_ids order; an edge only if its left cell is owned"""
    left = np.asarray(mesh.edge_cell_ids).reshape(-1, 2)[:, 0]
    owned = np.asarray(mesh.cell_is_owned)
    edges, bnds = [], []
    for b, boundary in enumerate(mesh.boundaries):
        if listed is not None and b not in listed:
            continue
        for e in np.asarray(boundary.edge_ids):
            if owned[left[e]]:
                edges.append(int(e))
                bnds.append(b)
    return np.array(edges, dtype=np.int32), np.array(bnds, dtype=np.int32)


def ghost_left_edges(mesh):
    left = np.asarray(mesh.edge_cell_ids).reshape(-1, 2)[:, 0]
    all_edges = np.concatenate([np.asarray(b.edge_ids) for b in mesh.boundaries])
    return int((np.asarray(mesh.cell_is_owned)[left[all_edges]] == 0).sum()), all_edges.size


def listings(mesh):
    nb = len(mesh.boundaries)
    assert nb >= 3
    return {"all": None, "subset": [nb - 1, 1], "none": []}


@pytest.mark.parametrize("which", ["all", "subset", "none"])
@pytest.mark.parametrize("name", MESHES)
def test_plan_is_the_references_loops(name, which):
    mesh = _mesh(name, False)
    listed = listings(mesh)[which]
    edges, bnds = plan_series_boundary_edges(mesh, listed)
    ref_e, ref_b = numpy_plan(mesh, listed)
    assert np.array_equal(edges, ref_e) and np.array_equal(bnds, ref_b)
    ghosts, K = ghost_left_edges(mesh)
    if which == "all":
        assert edges.size == K - ghosts
        # the boundary edges behind a ghost cell: none on the whole meshes, 1 on the interleaved part, 23 of 98 on the quad part
        assert ghosts == {"tri-prefix": 0, "quad-prefix": 0, "tri-o2l": 1, "quad-odd": 23}[name] and (name != "quad-odd" or K == 98)
        left = np.asarray(mesh.edge_cell_ids).reshape(-1, 2)[:, 0]
        assert np.asarray(mesh.cell_is_owned)[left[edges]].all()
    elif which == "subset":
        assert 0 < edges.size < K - ghosts and set(bnds) <= set(listed) and np.all(np.diff(bnds) >= 0)
    else:
        assert edges.size == 0


def test_plan_argument_errors():
    lib = _lib.load()
    mesh = _mesh("quad-odd", False)
    cfg, m, nb, barr, _, _keep = O._abi_arguments(RDyFlowConfig(), mesh, None)
    n = C.c_int32(-5)
    for bad in ([nb], [-1], [0, nb + 3]):
        listed = (C.c_int32 * len(bad))(*bad)
        assert lib.rdyhip_series_plan_boundary_edges(C.byref(m), nb, barr, len(bad), listed, C.byref(n), None, None) == 83
        assert b"boundary index" in lib.rdyhip_last_error()
    listed = (C.c_int32 * 1)(0)
    assert lib.rdyhip_series_plan_boundary_edges(C.byref(m), nb, barr, -1, listed, C.byref(n), None, None) == 83
    assert lib.rdyhip_series_plan_boundary_edges(C.byref(m), nb, barr, 1, listed, None, None, None) == 83
    assert n.value == -5
    # the count alone; a boundary named twice counts once
    twice = (C.c_int32 * 3)(0, 0, 0)
    assert lib.rdyhip_series_plan_boundary_edges(C.byref(m), nb, barr, 3, twice, C.byref(n), None, None) == 0
    assert n.value == numpy_plan(mesh, [0])[0].size


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("series_plan_dump")), "series_plan_dump")
    # the sanitizer runtimes linked into the program (clang++ does so by itself): it runs whatever else the environment preloads
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx] + FLAGS + static + [f"-I{ROOT}/include", f"-I{ROOT}/rdycore_amd/csrc", "-o", exe, SOURCE])
    return exe


@pytest.mark.parametrize("which", ["all", "subset", "none"])
@pytest.mark.parametrize("name", MESHES)
def test_plan_header_runs_clean_under_sanitizers(program, tmp_path, name, which):
    assert "-fsanitize=address,undefined" in FLAGS
    mesh = _mesh(name, False)
    listed = listings(mesh)[which]
    path = str(tmp_path / "case.bin")
    write_case(path, RDyFlowConfig(), mesh)
    arg = which if listed is None or not listed else ",".join(str(b) for b in listed)
    r = subprocess.run([program, path, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout)
    ref_e, ref_b = numpy_plan(mesh, listed)
    assert out["rc"] == 0 and out["num_edges"] == ref_e.size
    assert out["edge"] == ref_e.tolist() and out["boundary"] == ref_b.tolist()
    # slot[k]: the row of boundary edge k (all boundaries concatenated) in a record, or -1
    all_edges = np.concatenate([np.asarray(b.edge_ids) for b in mesh.boundaries])
    slot = np.array(out["slot"])
    assert slot.size == all_edges.size and np.array_equal(np.sort(slot[slot >= 0]), np.arange(ref_e.size))
    assert np.array_equal(all_edges[slot >= 0][np.argsort(slot[slot >= 0])], ref_e)
    assert abs(out["len_sum"] - float(np.asarray(mesh.edge_lengths)[all_edges].sum())) <= 1e-9 * all_edges.size


def test_plan_program_reports_a_bad_list_with_the_librarys_code_and_no_sanitizer_report(program, tmp_path):
    mesh = _mesh("quad-odd", False)
    path = str(tmp_path / "case.bin")
    write_case(path, RDyFlowConfig(), mesh)
    r = subprocess.run([program, path, f"0,{len(mesh.boundaries)}"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 83 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    assert json.loads(r.stdout)["rc"] == 83 and "boundary index" in json.loads(r.stdout)["error"]


# ---- the kernels in the code object --------------------------------------------------------------------------------------------

def test_series_kernels_are_in_the_code_object_without_scratch():
    pytest.importorskip("msgpack")
    from rdycore_amd import codeobj
    res = codeobj.kernel_resources(build.lib_path())
    for kernel in ("series_boundary_record_kernel", "series_observe_kernel"):
        forms = {k: v for k, v in res.items() if f"rdyhip::{kernel}" in k}
        assert len(forms) == 1, (kernel, sorted(forms))
        for k, v in forms.items():
            assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["lds"] == 0, (k, v)
    # the RHS kernels are what they were: 84 tiled / fused instantiations + 4 cell-centric ones
    assert sum("swe_rhs_tiled_kernel<" in k or "swe_rhs_muscl_fused_kernel<" in k for k in res) == 84
    assert sum("swe_rhs_kernel<" in k for k in res) == 4


# ---- the stepper's call sequence -----------------------------------------------------------------------------------------------

SERIES_CALLS = ("enable_obs", "enable_bf", "add_time", "record", "info", "read", "clear", "device_log", "edges")


class SeriesRecordingOp(RecordingOp):
    """RecordingOp with the series calls, recorded in the same log"""

    def enable_observation_series(self, owned_cell_ids, capacity):
        self.log.append(("enable_obs", tuple(owned_cell_ids), capacity))

    def enable_boundary_flux_series(self, capacity, boundaries=None):
        self.log.append(("enable_bf", capacity, boundaries))

    def series_add_time(self, dt):
        self.log.append(("add_time", dt))

    def series_record(self, kind, time, u_local=None):
        self.log.append(("record", kind, time, u_local, None if u_local is None else u_local.clone()))

    def series_read(self, kind, first=0, count=None):
        self.log.append(("read", kind))
        return "times", "values"

    def series_clear(self, kind):
        self.log.append(("clear", kind))


@pytest.mark.parametrize("temporal,fused", [("euler", True), ("euler", False), ("rk4", True), ("rk4", False)])
def test_without_series_the_stepper_makes_none_of_the_series_calls(temporal, fused):
    op = SeriesRecordingOp(3)
    u = torch.ones((3, 3), dtype=torch.float64)
    st = EulerStepper(op, temporal=temporal, fused=fused)
    assert st.series is None
    st.advance(u, 0.3, 1.0)
    st.advance(u, 0.3, 1.0)
    assert st.step == 8 and op.named(*SERIES_CALLS) == []


def test_only_the_series_that_are_on_are_enabled():
    op = SeriesRecordingOp(3)
    EulerStepper(op, series=TimeSeries(observation_sites=(2, 0, 2), observation_interval=2, capacity=9))
    assert op.log == [("enable_obs", (2, 0, 2), 9)]
    op = SeriesRecordingOp(3)
    EulerStepper(op, series=TimeSeries(boundary_flux_interval=1, boundaries=[1], capacity=5))
    assert op.log == [("enable_bf", 5, [1])]
    op = SeriesRecordingOp(3)
    EulerStepper(op, series=TimeSeries())
    assert op.log == []


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("temporal,fused", [("euler", True), ("euler", False), ("rk4", True)], ids=["euler_fused", "euler_unfused", "rk4"])
def test_stepper_plays_write_time_series(temporal, fused, interval):
    """0.3 + 0.3 + 0.3 + 0.1, twice: a shortened last step in either advance().  One monitor call at step 0 and one after every
    step; in each: observations (step % interval == 0), add_time(the interval's dt), boundary record (step % interval == 0)."""
    op = SeriesRecordingOp(3)
    u = torch.ones((3, 3), dtype=torch.float64)
    st = EulerStepper(op, temporal=temporal, fused=fused,
                      series=TimeSeries(observation_sites=(1,), observation_interval=interval, boundary_flux_interval=interval, capacity=16))
    assert op.log == [("enable_obs", (1,), 16), ("enable_bf", 16, None)]
    op.log.clear()
    st.advance(u, 0.3, 1.0)
    st.advance(u, 0.3, 1.0)
    assert st.step == 8
    step_names = {("euler", True): ("euler",), ("euler", False): ("axpy",), ("rk4", True): ("rk4",)}[(temporal, fused)]
    # split the log into monitor calls: the series calls between two steps
    monitors, cur, hs = [], [], []
    for e in op.log:
        if e[0] in step_names:
            monitors.append(cur)
            cur = []
            hs.append(e[1])
        elif e[0] in SERIES_CALLS:
            cur.append(e)
    monitors.append(cur)
    assert len(hs) == 8 and len(monitors) == 9 and hs[3] < 0.3 and hs[7] < 0.3 and hs[0] == 0.3
    times = np.concatenate([[0.0], np.cumsum(hs)])
    for step, calls in enumerate(monitors):
        want = ["add_time"]
        if step % interval == 0:
            want = ["record", "add_time", "record"]
        assert [c[0] for c in calls] == want, (step, calls)
        add = [c for c in calls if c[0] == "add_time"][0]
        assert add[1] == 0.3                                     # the interval's dt, also after the steps of 0.1
        if step % interval == 0:
            obs, bf = calls[0], calls[2]
            assert obs[1] == O.SERIES_OBSERVATIONS and bf[1] == O.SERIES_BOUNDARY_FLUXES and bf[3] is None
            assert abs(obs[2] - times[step]) <= 1e-12 and abs(bf[2] - times[step]) <= 1e-12
            # the current state: what du/dt = lam u has become after `step` steps (rk4's stand-in step does nothing)
            expect = 1.0 if temporal == "rk4" else float(np.prod([1.0 + h * op.lam for h in hs[:step]]))
            assert obs[3] is not None and torch.allclose(obs[4], torch.full((3, 3), expect, dtype=torch.float64), rtol=1e-14, atol=0)
    assert len(op.named("record")) == 2 * len([s for s in range(9) if s % interval == 0])


def test_boundary_series_alone_and_different_intervals():
    op = SeriesRecordingOp(3)
    u = torch.ones((3, 3), dtype=torch.float64)
    st = EulerStepper(op, series=TimeSeries(observation_sites=(0,), observation_interval=2, boundary_flux_interval=3, capacity=16))
    op.log.clear()
    st.advance(u, 0.25, 1.5)                                      # six steps
    rec = op.named("record")
    assert [(e[1], round(e[2] / 0.25)) for e in rec] == [(1, 0), (2, 0), (1, 2), (2, 3), (1, 4), (1, 6), (2, 6)]
    assert len(op.named("add_time")) == 7
    assert st.series_read(O.SERIES_BOUNDARY_FLUXES, clear=True) == ("times", "values")
    assert op.log[-2:] == [("read", 2), ("clear", 2)]
