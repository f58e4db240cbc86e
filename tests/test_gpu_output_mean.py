"""GPU: the time-averaged output fields kept on the device (rdyhip_output_mean_*, csrc/output_kernels.h) against the loop they
replace -- a host that takes the primitive-variables and the source pointer and runs three rdyhip_axpy_owned launches per step
into arrays of its own -- bit for bit, and against numpy's sum(dt * inst) / sum(dt) over the oracle's fields.

Meshes: test_gpu_kernel_matrix.matrix_mesh (a few thousand cells) as tri-prefix, quad-prefix and tri-o2l (the owned index is
not the local one), and one part of 567 owned quads with 21 ghosts behind them: the owned rows are a prefix, n_owned is odd and
no multiple of 256, so the last workgroup of the accumulate kernel is partial and the 16-byte form of the mean kernel ends in
its scalar tail (3 * n_owned is odd).
States: random_case with dry cells and cells at tiny_h, as tests/test_gpu_pv_on_demand.py builds them; a nonzero water source
through the ordinary setter, momentum sources zero (the water-only mode of the source).  Three steps with three different dt.
Tolerance against the oracle: the bar of test_gpu_parity.py (TOL, rel L-inf against max(1, |ref|)).

The states must stay finite for three steps, or "equal" means nothing.  First order takes the square root of a negative depth as
the reference does (NaN), and random_case's states get there at once: sources that evaporate dry cells, and supercritical flow
receding from an exactly dry cell, which the third Runge-Kutta stage leaves a hair below zero whatever dt is (the oracle loop
shows both on the CPU).  So the rain is positive, the momenta are a tenth of random_case's (h is untouched: the dry cells, the
films and the cells at tiny_h stay) and the steps are 0.1 - 0.25 ms; the oracle test asserts that its reference is finite.
"Bit for bit" compares the 64-bit patterns (-0.0 is not +0.0).
Every test runs behind both kernel variants (tests/conftest.py); hydrostatic reconstruction lives in the tiled kernels only."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from rdycore_amd import build
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd._lib import RDyHipError
from rdycore_amd.operator import OUTPUT_PRIMITIVE_VARIABLES, OUTPUT_SOLUTION, OUTPUT_SOURCES, Operator, RDyFlowConfig

from helpers import oracle_from_case, rel_linf
from random_cases import random_case, random_connectivity
from test_gpu_c_client import compile_client, write_case
from test_gpu_kernel_matrix import matrix_mesh
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

ALL = OUTPUT_SOLUTION | OUTPUT_PRIMITIVE_VARIABLES | OUTPUT_SOURCES
VARS = (OUTPUT_SOLUTION, OUTPUT_PRIMITIVE_VARIABLES, OUTPUT_SOURCES)
NAMES = {OUTPUT_SOLUTION: "solution", OUTPUT_PRIMITIVE_VARIABLES: "primitive variables", OUTPUT_SOURCES: "sources"}
MESHES = ["tri-prefix", "quad-prefix", "tri-o2l", "quad-odd"]
PATHS = ["euler_fused", "rhs_axpy", "rk4"]
DTS = (1e-4, 2.5e-4, 1.5e-4)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(a):
    return _torch().tensor(a, dtype=_torch().float64, device="cuda")


@functools.lru_cache(maxsize=None)
def _odd_mesh(project_2d):
    rng = np.random.default_rng(31)
    nx, ny = 28, 21
    xyz, conn = random_connectivity(rng, "quad", nx, ny)
    owned = (np.arange(nx * ny) % nx) < nx - 1                      # the last column: ghosts, numbered behind the owned cells
    mesh = M.extract_local_mesh(xyz, conn, owned, boundary_classifier=M.box_side_boundaries(0, nx, 0, ny), project_2d=project_2d)
    assert mesh.num_owned_cells == 567 and mesh.num_cells == 588
    return mesh


def _mesh(name, hr):
    if name == "quad-odd":
        return _odd_mesh(hr)
    kind, layout = name.split("-")
    return matrix_mesh(kind, layout, hr)


@functools.lru_cache(maxsize=None)
def _case(name, hr, seed_offset=0):
    rng = np.random.default_rng(9100 + 10 * MESHES.index(name) + int(hr) + 1000 * seed_offset)
    mesh = _mesh(name, hr)
    cfg = RDyFlowConfig(tiny_h=1e-5, source_method=int(rng.integers(0, 2)), well_balancing=2 if hr else 0)
    case = random_case(rng, mesh, cfg, region_block=64)
    ids = rng.permutation(mesh.num_cells)[:16]                      # a few cells at h == tiny_h exactly, moving
    case.u_local[ids, 0] = cfg.tiny_h
    case.u_local[ids, 1:] = rng.normal(size=(16, 2)) * 1e-6
    case.u_local[:, 1:] *= 0.1                                      # see the module docstring: the states stay finite
    # rain only: the source stays in its water-only mode, and no dry cell is drawn below zero depth
    case.ext_src[:, 0] = np.abs(case.ext_src[:, 0])
    case.ext_src[:, 1:] = 0.0
    assert case.ext_src[:, 0].min() > 0.0
    return case


def _own(case):
    return _torch().as_tensor(np.asarray(case.mesh.cell_owned_to_local), device="cuda", dtype=_torch().int64)


class _HostLoop:
    """the parent's way: both pointers taken, three axpy_owned launches into zeroed local-size arrays"""

    def __init__(self, op, case):
        torch = _torch()
        self.op, self.own = op, _own(case)
        self.pv = op.primitive_variables
        self.src = op.external_sources
        self.acc = {v: torch.zeros((case.mesh.num_cells, 3), dtype=torch.float64, device="cuda") for v in VARS}
        self.T = {v: 0.0 for v in VARS}

    def accumulate(self, vars, dt, u_local=None):
        inst = {OUTPUT_SOLUTION: (lambda: u_local.index_select(0, self.own)), OUTPUT_PRIMITIVE_VARIABLES: (lambda: self.pv),
                OUTPUT_SOURCES: (lambda: self.src)}
        for v in VARS:
            if vars & v:
                self.op.axpy_owned(dt, inst[v](), self.acc[v])
                self.T[v] += dt

    def mean(self, v):
        return self.acc[v].index_select(0, self.own) * (1.0 / self.T[v]), self.T[v]


class _NewCalls:
    def __init__(self, op, case):
        self.op = op
        op.enable_output_means(ALL)

    def accumulate(self, vars, dt, u_local=None):
        self.op.accumulate_output_means(vars, dt, u_local)

    def mean(self, v):
        return self.op.output_mean(v)


def _three_steps(op, case, path, acc):
    """DTS on `path`, accumulating through `acc` where the stepper would; what a caller sees of every step, and the means"""
    torch = _torch()
    no = case.mesh.num_owned_cells
    u = _dev(case.u_local)
    u2 = u.clone()
    steps = []
    for k, dt in enumerate(DTS):
        f = None
        if path == "euler_fused":
            f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda") if k != 1 else None     # the middle step never writes F
            op.euler_step(dt, u, u2, f)
            acc.accumulate(ALL, dt, u2)
            u, u2 = u2, u
        elif path == "rhs_axpy":
            f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")
            op.rhs_function(dt, u, f)
            acc.accumulate(OUTPUT_PRIMITIVE_VARIABLES | OUTPUT_SOURCES, dt)
            op.axpy_owned(dt, f, u)
            acc.accumulate(OUTPUT_SOLUTION, dt, u)
        else:
            op.rk4_step(dt, u)
            acc.accumulate(ALL, dt, u)
        op.update_diagnostics()
        steps.append((f, u.clone(), op.get_diagnostics().max_courant_num))
    means = {v: acc.mean(v) for v in VARS}
    torch.cuda.synchronize()
    return steps, means


def _skip_hr_behind_the_cell_kernel(hr, rdyhip_kernel):
    if hr and rdyhip_kernel == "cell":
        pytest.skip("hydrostatic reconstruction is implemented by the tiled kernel")


@functools.lru_cache(maxsize=None)
def _new_path_run(name, hr, path, kernel):
    """operator B: the new calls, no pointer taken.  Run once per (mesh, order, path, kernel variant -- the fixture has set
    it), shared by the tests below."""
    assert os.environ.get("RDYHIP_KERNEL") == kernel
    case = _case(name, hr)
    op = CS.create_operator(case)
    water_only = op.source_is_water_only()
    assert water_only
    steps, means = _three_steps(op, case, path, _NewCalls(op, case))
    assert not op.primitive_variables_stored(), "the accumulate calls turned the primitive-variable stores on"
    assert op.source_is_water_only() == water_only, "the accumulate calls changed the mode of the source"
    op.destroy()
    return steps, means


def _same_bits(a, b):
    """finite, and the same 64 bits"""
    torch = _torch()
    return a.shape == b.shape and bool(torch.isfinite(a).all()) and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _assert_same_means(a, b, what):
    for v in VARS:
        (ma, ta), (mb, tb) = a[v], b[v]
        assert ta == tb, f"{what}: accumulated time of the {NAMES[v]}: {ta!r} / {tb!r}"
        assert _same_bits(ma, mb), f"{what}: mean of the {NAMES[v]} differs, max |diff| {float((ma - mb).abs().max()):.3e}"


# ---- 1. bit for bit against the loop it replaces -------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
@pytest.mark.parametrize("name", MESHES)
def test_means_are_the_bits_of_the_host_loop(name, hr, path, rdyhip_kernel):
    torch = _torch()
    _skip_hr_behind_the_cell_kernel(hr, rdyhip_kernel)
    case = _case(name, hr)
    what = f"{name}-{'hr' if hr else 'plain'}-{path}"
    a = CS.create_operator(case)
    host = _HostLoop(a, case)
    assert a.primitive_variables_stored() and not a.source_is_water_only()
    steps_a, means_a = _three_steps(a, case, path, host)
    a.destroy()
    steps_b, means_b = _new_path_run(name, hr, path, rdyhip_kernel)
    _assert_same_means(means_a, means_b, what)
    for k, ((fa, ua, ca), (fb, ub, cb)) in enumerate(zip(steps_a, steps_b)):
        assert (fa is None) == (fb is None) and (fa is None or _same_bits(fa, fb)), f"{what}: F of step {k}"
        assert _same_bits(ua, ub), f"{what}: state after step {k}"
        assert ca == cb > 0.0, f"{what}: Courant number of step {k}: {ca} / {cb}"
    assert abs(means_b[OUTPUT_SOLUTION][1] - sum(DTS)) <= 1e-15


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_means(name, hr, path):
    case = _case(name, hr)
    orc = oracle_from_case(case)
    own = np.asarray(case.mesh.cell_owned_to_local)
    u = case.u_local.copy()
    acc = {v: np.zeros((case.mesh.num_owned_cells, 3)) for v in VARS}

    def rhs(dt, state):
        orc.reset_diagnostics()
        return orc.apply(dt, state)
    for dt in DTS:
        if path == "rk4":
            k = []
            for a in (0.0, 0.5, 0.5, 1.0):
                y = u.copy()
                if k:
                    y[own] += a * dt * k[-1]
                k.append(rhs(dt, y).copy())
            u[own] += dt * (k[0] / 6.0 + k[1] / 3.0 + k[2] / 3.0 + k[3] / 6.0)
        else:
            u[own] += dt * rhs(dt, u)
        acc[OUTPUT_PRIMITIVE_VARIABLES] += dt * orc.primitive_variables     # of the state the last evaluation saw
        acc[OUTPUT_SOLUTION] += dt * u[own]
        acc[OUTPUT_SOURCES] += dt * case.ext_src
    return {v: acc[v] / sum(DTS) for v in VARS}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
@pytest.mark.parametrize("name", MESHES)
def test_means_match_the_oracle(name, hr, path, rdyhip_kernel):
    _torch()
    _skip_hr_behind_the_cell_kernel(hr, rdyhip_kernel)
    _, means = _new_path_run(name, hr, path, rdyhip_kernel)
    ref = _oracle_means(name, hr, path)
    got = {v: means[v][0].cpu().numpy() for v in VARS}
    assert all(np.isfinite(ref[v]).all() for v in VARS), "the oracle loop left the finite numbers: the test's states are not fit for three steps"
    errs = {v: rel_linf(got[v], ref[v]) for v in VARS}
    print(f"{name}-{'hr' if hr else 'plain'}-{path}: rel L-inf " + ", ".join(f"{NAMES[v]} {errs[v]:.3e}" for v in VARS))
    for v in VARS:
        assert np.isfinite(got[v]).all() and errs[v] <= TOL, f"mean of the {NAMES[v]}: rel L-inf {errs[v]:.3e}"
    assert np.abs(ref[OUTPUT_PRIMITIVE_VARIABLES][:, 1:]).max() > 0.1 and ref[OUTPUT_SOURCES][:, 0].min() > 0.0


# ---- 3. windows and errors -----------------------------------------------------------------------------------------------------

def _raises_user_error(call):
    with pytest.raises(RDyHipError) as e:
        call()
    assert e.value.code == 83, e.value
    return e.value


def test_windows():
    torch = _torch()
    case, other = _case("quad-odd", False), _case("quad-odd", False, seed_offset=1)
    no = case.mesh.num_owned_cells
    u1, u2 = _dev(case.u_local), _dev(other.u_local)
    f = torch.empty((no, 3), dtype=torch.float64, device="cuda")
    op, fresh = CS.create_operator(case), CS.create_operator(case)
    op.enable_output_means(ALL)
    fresh.enable_output_means(ALL)
    # first window: two accumulates of the first state
    op.rhs_function(DTS[0], u1, f)
    op.accumulate_output_means(ALL, DTS[0], u1)
    op.accumulate_output_means(ALL, DTS[1], u1)
    first = {v: op.output_mean(v) for v in VARS}
    assert all(first[v][1] == DTS[0] + DTS[1] and op.output_mean_time(v) == DTS[0] + DTS[1] for v in VARS)
    # enable again: the content stays
    op.enable_output_means(ALL)
    _assert_same_means(first, {v: op.output_mean(v) for v in VARS}, "after a second enable")
    # get resets nothing; reset does
    op.reset_output_means(ALL)
    for v in VARS:
        assert op.output_mean_time(v) == 0.0
        err = _raises_user_error(lambda: op.output_mean(v))
        assert "no time" in err.message
    # the second window knows nothing of the first: the bits of an operator that never had one
    for o in (op, fresh):
        o.rhs_function(DTS[2], u2, f)
        o.accumulate_output_means(ALL, DTS[2], u2)
    second, ref = {v: op.output_mean(v) for v in VARS}, {v: fresh.output_mean(v) for v in VARS}
    torch.cuda.synchronize()
    _assert_same_means(second, ref, "second window")
    assert not _same_bits(second[OUTPUT_SOLUTION][0], first[OUTPUT_SOLUTION][0])
    # one variable reset, the others keep their window
    op.reset_output_means(OUTPUT_SOURCES)
    assert op.output_mean_time(OUTPUT_SOURCES) == 0.0 and op.output_mean_time(OUTPUT_SOLUTION) == DTS[2]
    op.destroy()
    fresh.destroy()


def test_errors_and_device_bytes():
    torch = _torch()
    case = _case("quad-odd", False)
    no = case.mesh.num_owned_cells
    u = _dev(case.u_local)
    op = CS.create_operator(case)
    b0 = op.layout_info()["device_bytes"]
    _raises_user_error(lambda: op.accumulate_output_means(OUTPUT_SOLUTION, 0.1, u))       # nothing is enabled yet
    _raises_user_error(lambda: op.output_mean(OUTPUT_SOLUTION))
    _raises_user_error(lambda: op.output_mean_time(OUTPUT_SOLUTION))
    op.enable_output_means(OUTPUT_SOLUTION)
    assert op.layout_info()["device_bytes"] - b0 == 24 * no
    op.accumulate_output_means(OUTPUT_SOLUTION, 0.25, u)
    # a variable that is not enabled: 83, and no time changes -- not even that of the enabled one named beside it
    err = _raises_user_error(lambda: op.accumulate_output_means(OUTPUT_SOLUTION | OUTPUT_SOURCES, 0.5, u))
    assert "not enabled" in err.message
    assert op.output_mean_time(OUTPUT_SOLUTION) == 0.25
    _raises_user_error(lambda: op.reset_output_means(OUTPUT_SOURCES))
    # unknown bits, more or less than one variable where one is needed, a missing state array
    _raises_user_error(lambda: op.enable_output_means(8))
    _raises_user_error(lambda: op.accumulate_output_means(9, 0.5, u))
    _raises_user_error(lambda: op.output_mean(3))
    _raises_user_error(lambda: op.output_mean(0))
    _raises_user_error(lambda: op.output_mean_time(5))
    _raises_user_error(lambda: op.accumulate_output_means(OUTPUT_SOLUTION, 0.5, None))
    assert op.output_mean_time(OUTPUT_SOLUTION) == 0.25
    op.enable_output_means(ALL)
    assert op.layout_info()["device_bytes"] - b0 == 3 * 24 * no
    op.enable_output_means(ALL)
    assert op.layout_info()["device_bytes"] - b0 == 3 * 24 * no
    mean, t = op.output_mean(OUTPUT_SOLUTION)                                             # the content survived both enables
    torch.cuda.synchronize()
    assert t == 0.25 and torch.equal(mean, (0.25 * u[:no]) * (1.0 / 0.25))
    op.destroy()


def test_before_any_evaluation_the_primitive_variables_are_zeros():
    torch = _torch()
    case = _case("tri-o2l", False)
    op = CS.create_operator(case)
    op.enable_output_means(ALL)
    u = _dev(case.u_local)
    op.accumulate_output_means(ALL, 0.5, u)
    mean, t = op.output_mean(OUTPUT_PRIMITIVE_VARIABLES)
    sol, _ = op.output_mean(OUTPUT_SOLUTION)
    torch.cuda.synchronize()
    assert t == 0.5 and mean.shape == (case.mesh.num_owned_cells, 3) and torch.all(mean == 0.0)
    assert torch.equal(sol, u.index_select(0, _own(case)))                                # 0.5 u * 2: exact
    assert not op.primitive_variables_stored()
    op.destroy()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,hr", [("quad-odd", False), ("tri-o2l", True)], ids=["quad-odd-plain", "tri-o2l-hr"])
def test_with_the_pointer_handed_out_the_stored_rows_are_read(name, hr, path, rdyhip_kernel):
    """storing on: the accumulate reads d_pv back instead of forming (h, u, v) -- the same bits"""
    _skip_hr_behind_the_cell_kernel(hr, rdyhip_kernel)
    case = _case(name, hr)
    op = CS.create_operator(case)
    pv = op.primitive_variables
    assert op.primitive_variables_stored()
    steps, means = _three_steps(op, case, path, _NewCalls(op, case))
    assert op.primitive_variables_stored() and op.source_is_water_only()
    op.destroy()
    _assert_same_means(means, _new_path_run(name, hr, path, rdyhip_kernel)[1], f"{name}-{path}, storing")
    del pv


# ---- 4. source modes -----------------------------------------------------------------------------------------------------------

def test_source_mean_is_the_same_in_and_out_of_the_water_only_mode():
    torch = _torch()
    case = _case("quad-odd", False)
    a, b = CS.create_operator(case), CS.create_operator(case)
    src = b.external_sources                                   # rdyhip_field_ptr: ends the mode for the life of the operator
    assert a.source_is_water_only() and not b.source_is_water_only()
    for op in (a, b):
        op.enable_output_means(OUTPUT_SOURCES)
        for dt in DTS:
            op.accumulate_output_means(OUTPUT_SOURCES, dt)
    (ma, ta), (mb, tb) = a.output_mean(OUTPUT_SOURCES), b.output_mean(OUTPUT_SOURCES)
    torch.cuda.synchronize()
    assert ta == tb and torch.equal(ma, mb)
    assert a.source_is_water_only() and not b.source_is_water_only()
    mom = ma[:, 1:]
    assert torch.all(mom == 0.0) and not torch.signbit(mom).any(), "momentum components of the source mean are not +0.0"
    assert rel_linf(ma[:, 0].cpu().numpy(), case.ext_src[:, 0]) <= TOL and torch.equal(src[:, 0], _dev(case.ext_src[:, 0]))
    a.destroy()
    b.destroy()


# ---- 5. the stepper ------------------------------------------------------------------------------------------------------------

def _interval_steps(time, dt, interval):
    """the step sizes EulerStepper.advance takes from `time` (TS_EXACTFINALTIME_MATCHSTEP)"""
    t_end, hs = time + interval, []
    while time < t_end * (1.0 - 1e-14):
        hs.append(min(dt, t_end - time))
        time += hs[-1]
    return hs, time


@pytest.mark.parametrize("temporal,fused", [("euler", True), ("euler", False), ("rk4", True)], ids=["euler_fused", "euler_unfused", "rk4"])
def test_stepper_makes_the_explicit_call_sequence(temporal, fused):
    torch = _torch()
    from rdycore_amd.timestep import EulerStepper
    case = _case("quad-prefix", False)                         # no ghost cells: without a halo the stepper's second array has none to fill
    assert case.mesh.num_cells == case.mesh.num_owned_cells
    no = case.mesh.num_owned_cells
    dt, interval = 2e-4, 5e-4                                  # 0.2 + 0.2 + 0.1 ms: a shortened last step, accumulated with 0.2 ms
    # the stepper
    a = CS.create_operator(case)
    ua = _dev(case.u_local)
    st = EulerStepper(a, temporal=temporal, fused=fused, means=ALL)
    # the explicit sequence
    b = CS.create_operator(case)
    b.enable_output_means(ALL)
    ub = _dev(case.u_local)
    u2, f = ub.clone(), torch.empty((no, 3), dtype=torch.float64, device="cuda")
    time = 0.0
    for window in range(2):
        assert st.advance(ua, dt, interval) == dt
        hs, time = _interval_steps(time, dt, interval)
        assert len(hs) == 3 and hs[2] < dt
        if window == 0:
            b.accumulate_output_means(ALL, dt, ub)             # the monitor's call at step 0
        b.reset_diagnostics()
        cur, nxt = ub, u2
        for h in hs:
            if temporal == "rk4":
                b.rk4_step(h, ub)
                b.accumulate_output_means(ALL, dt, ub)
            elif fused:
                b.euler_step(h, cur, nxt)
                b.accumulate_output_means(ALL, dt, nxt)
                cur, nxt = nxt, cur
            else:
                b.rhs_function(h, ub, f)
                b.accumulate_output_means(OUTPUT_PRIMITIVE_VARIABLES | OUTPUT_SOURCES, dt)
                b.axpy_owned(h, f, ub)
                b.accumulate_output_means(OUTPUT_SOLUTION, dt, ub)
        if cur is not ub:
            ub.copy_(cur)
        n_acc = len(hs) + (1 if window == 0 else 0)
        for v in VARS:
            ma, ta = st.output_mean(v)                         # get + reset: a new window
            mb, tb = b.output_mean(v)
            b.reset_output_means(v)
            torch.cuda.synchronize()
            assert ta == tb and abs(ta - n_acc * dt) <= 1e-15, (window, NAMES[v], ta, tb)
            assert _same_bits(ma, mb), f"window {window}: mean of the {NAMES[v]}"
            assert a.output_mean_time(v) == 0.0
        assert _same_bits(ua, ub)
    assert st.step == 6 and not a.primitive_variables_stored() and a.source_is_water_only()
    a.destroy()
    b.destroy()


# ---- 6. the C host -------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_c_host_keeps_the_means(tmp_path):
    """tests/c_client/rdyhip_mean_client.c: four fused Euler steps with all three variables accumulated = the same calls from
    Python, bit for bit"""
    torch = _torch()
    build.build_native()
    K = 2 * np.pi / 23
    mesh = M.structured_tri_mesh(31, 19, 1.0, zfunc=CS.mms_bathymetry(K=K), order="tiled", tile=4)
    case = CS.friction_slope_case(mesh, 31, 19, dt=1e-2, source_method=1, K=K)
    no = mesh.num_owned_cells
    path, out_path = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(path, case, True, np.zeros((no, 3)), np.zeros((no, 3)), np.zeros((no, 3)), 0.0)
    exe = compile_client(tmp_path, "rdyhip_mean_client")
    env = dict(os.environ)
    env.pop("RDYHIP_LIB", None)
    n, dt = 4, 5e-3
    run = subprocess.run([exe, path, out_path, str(n), repr(dt)], capture_output=True, text=True, env=env, timeout=100)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = open(out_path, "rb").read()
    steps, = struct.unpack("q", raw[:8])
    t_c, = struct.unpack("d", raw[8:16])
    means_c = np.frombuffer(raw[16:], dtype=np.float64).reshape(3, no, 3)
    op = CS.create_operator(case)
    op.enable_output_means(ALL)
    u = _dev(case.u_local)
    u2 = u.clone()
    for _ in range(n):
        op.euler_step(dt, u, u2)
        op.accumulate_output_means(ALL, dt, u2)
        u, u2 = u2, u
    assert steps == n
    for i, v in enumerate(VARS):
        mean, t = op.output_mean(v)
        torch.cuda.synchronize()
        assert t == t_c
        assert np.isfinite(means_c[i]).all() and np.array_equal(mean.cpu().numpy().view(np.int64), means_c[i].view(np.int64)), f"mean of the {NAMES[v]}: C host and Python differ"
    assert np.abs(means_c[1][:, 1:]).max() > 0.0
    op.destroy()


# ---- 7. a rank that owns nothing -----------------------------------------------------------------------------------------------

def test_rank_that_owns_nothing():
    torch = _torch()
    xyz, conn, _, _ = M.structured_tri_connectivity(3, 2)
    mesh = M.build_mesh(xyz, conn, is_owned=np.zeros(conn.shape[0], dtype=np.int32), boundary_classifier=M.box_side_boundaries(0, 3, 0, 2))
    assert mesh.num_owned_cells == 0
    op = Operator.create(RDyFlowConfig(), mesh)
    u = torch.ones((mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    f = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    b0 = op.layout_info()["device_bytes"]
    op.enable_output_means(ALL)
    assert op.layout_info()["device_bytes"] == b0
    op.accumulate_output_means(ALL, 0.25, u)
    op.rhs_function(0.1, u, f)
    op.accumulate_output_means(ALL, 0.5, u)
    op.accumulate_output_means(OUTPUT_SOURCES, 0.25)
    assert op.output_mean_time(OUTPUT_SOLUTION) == 0.75 and op.output_mean_time(OUTPUT_SOURCES) == 1.0
    for v in VARS:
        mean, t = op.output_mean(v)
        assert mean.shape == (0, 3) and t == (1.0 if v == OUTPUT_SOURCES else 0.75)
    op.reset_output_means(ALL)
    assert all(op.output_mean_time(v) == 0.0 for v in VARS)
    torch.cuda.synchronize()
    op.destroy()
