"""GPU: the non-blocking Courant read-back (rdyhip_diagnostics_begin / _ready / _wait, csrc/diagnostics_calls.h).

The reference throughout is the blocking call on the same device state (rdyhip_update_diagnostics, which test_gpu_parity.py,
test_gpu_numbering.py and test_gpu_cell_family_numbering.py tie to the oracle): begin + wait + get must deliver the same struct,
value bits and both ids.  The operator is given begin + wait FIRST and the blocking call second, so a wait that stored nothing
would leave the (0, -1, -1) of the evaluation's reset behind.  Shapes: 30 and 270 triangles (under one wave; one workgroup and a
partial wave), the 44 quads of planar_dam_10x5.msh, one rank's part of a random partition (ghosts interleaved with owned cells),
a rank that owns nothing."""
import functools
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from helpers import interior_courant_numbers, owned_side_courant_numbers
from random_cases import random_case
from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import Operator, RDyFlowConfig, RDyHipError, SOURCE_IMPLICIT_XQ2018, TRACER_RIEMANN_ROE
from rdycore_amd.timestep import AdaptiveTime, EulerStepper
from test_gpu_c_client import compile_client, write_case
from test_gpu_ensemble import _set_member, boundary_courant_numbers
from test_gpu_tracers import _empty_mesh, _mesh
from test_tracers_cpu import tracer_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMPTY = (0.0, -1, -1)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(a):
    return _torch().tensor(np.ascontiguousarray(a), dtype=_torch().float64, device="cuda")


def _bits(d):
    """a struct as (the value's bit pattern, edge id, cell id)"""
    return struct.unpack("<q", struct.pack("<d", float(d.max_courant_num)))[0], int(d.global_edge_id), int(d.global_cell_id)


def _async(op):
    op.diagnostics_begin()
    op.diagnostics_wait()
    return _bits(op.get_diagnostics())


def _blocking(op):
    op.update_diagnostics()
    return _bits(op.get_diagnostics())


def _code(call, *args):
    with pytest.raises(RDyHipError) as e:
        call(*args)
    return e.value.code


@functools.lru_cache(maxsize=None)
def _two_states(name="tri-270", second_order=False):
    """two random states of one configuration on one mesh (wet / dry / thin films, friction, slopes, sources)"""
    mesh = _mesh(name)
    cfg = RDyFlowConfig(second_order=second_order)
    block = 16 if name == "tri-270" else 0
    a = random_case(np.random.default_rng(4101), mesh, cfg, region_block=block)
    b = random_case(np.random.default_rng(4102), mesh, cfg, region_block=block)
    b.condition_types, b.boundary_values = a.condition_types, a.boundary_values
    return a, b


def _f(mesh, n=3):
    return _torch().empty((mesh.num_owned_cells, n), dtype=_torch().float64, device="cuda")


# ---- 1. the same result as the blocking call -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tri-30", "tri-270", "quad-44"])
def test_same_struct_after_rhs_function_and_euler_step(name):
    case, _ = _two_states(name)
    op = CS.create_operator(case)
    u, out = _dev(case.u_local), _dev(case.u_local)
    op.rhs_function(case.dt, u, _f(case.mesh))
    got, want = _async(op), _blocking(op)
    print(f"{name} rhs_function: {got} blocking {want}")
    assert got == want and want[0] != 0 and want[1] >= 0
    op.euler_step(case.dt, u, out)
    got, want = _async(op), _blocking(op)
    assert got == want and want[1] >= 0
    op.destroy()


def test_same_struct_on_a_second_order_operator(monkeypatch):
    monkeypatch.delenv("RDYHIP_KERNEL", raising=False)     # second order is the tiled kernels' alone: both runs of this test use them
    case, _ = _two_states("tri-270", True)
    op = CS.create_operator(case)
    op.rhs_function(case.dt, _dev(case.u_local), _f(case.mesh))
    got, want = _async(op), _blocking(op)
    assert got == want and want[1] >= 0
    op.destroy()


@functools.lru_cache(maxsize=None)
def _ghost_rank_case():
    """On one rank's part of a random partition (part-o2l): a tracer case whose flow state puts the largest Courant number on a
    cut edge whose GHOST cell has the smaller area -- a lake at rest of 1 m, with 50 m of water moving at 100 m/s along the
    edge's normal in the edge's two cells.  The reference's rule (src/swe/swe_petsc.c:294-295: the cell of the smaller area)
    names the ghost there, the owned-side rule of the tracer kernel the owned cell.  Returns (case, tracer reference, state
    [num_cells, 5], local ghost cell, local owned cell)."""
    mesh = _mesh("part-o2l")
    case, ref, u = tracer_case(np.random.default_rng(77), mesh, 2, TRACER_RIEMANN_ROE)
    e = np.asarray(mesh.edge_internal_ids)
    l, r = mesh.edge_cell_ids[2 * e], mesh.edge_cell_ids[2 * e + 1]
    own = mesh.cell_is_owned != 0
    o, g = np.where(own[l], l, r), np.where(own[l], r, l)
    case.dt = 1e-4
    for k in np.nonzero((own[l] != own[r]) & (mesh.cell_areas[g] < 0.8 * mesh.cell_areas[o]))[0]:
        uu = np.zeros((mesh.num_cells, 3))
        uu[:, 0] = 1.0
        for c in (o[k], g[k]):
            uu[c] = [50.0, 50.0 * 100.0 * mesh.edge_cn[e[k]], 50.0 * 100.0 * mesh.edge_sn[e[k]]]
        case.u_local = uu
        ci, cb = interior_courant_numbers(case), boundary_courant_numbers(case)
        top = np.sort(ci[np.isfinite(ci)])[-2:]
        # the edge stands alone at the top by the reference's rule (len / min(area), all local edges) and by the owned-side
        # restatement (len / area_self, edges of owned cells: the tracer kernel, and the cell-centric SWE kernel)
        c, _, edge, cell = owned_side_courant_numbers(mesh, ci, cb)
        s = np.argsort(c)
        if (np.nanargmax(ci) == k and top[1] > 1.5 * top[0] and top[1] > 1.5 * np.nanmax(cb)
                and edge[s[-1]] == e[k] and cell[s[-1]] == o[k] and c[s[-1]] > 1.2 * c[s[-2]]):
            conc = np.tile([0.3, 0.05], (mesh.num_cells, 1))
            return case, ref, np.concatenate([uu, uu[:, :1] * conc], axis=1), int(g[k]), int(o[k])
    raise AssertionError("no cut edge of the partition carries the state")


def _ghost_rank_operator():
    case, ref, u, g, o = _ghost_rank_case()
    op = CS.create_operator(case)
    op.enable_tracers(2, TRACER_RIEMANN_ROE)
    for j in range(2):
        op.tracers_set_source(j, ref.tracer_sources[:, j])
    for b in range(len(case.mesh.boundaries)):
        if case.mesh.boundaries[b].num_edges:
            op.tracers_set_boundary_values(b, ref.boundary_values[b])
    return op, case, _dev(u), g, o


def test_same_struct_after_a_tracer_evaluation_on_a_rank_with_ghosts():
    op, case, u, g, o = _ghost_rank_operator()
    mesh = case.mesh
    assert mesh.num_cells > mesh.num_owned_cells
    op.tracers_rhs_function(case.dt, u, _f(mesh, 5))
    got, want = _async(op), _blocking(op)
    print(f"tracers on part-o2l: {got} blocking {want}")
    assert got == want and want[2] == int(mesh.cell_global_ids[o])
    op.destroy()


def test_same_struct_on_an_exactly_tied_state():
    """a lake at rest on 270 equal triangles under a scrambled numbering: the edges of each of the three kinds tie bit for bit"""
    mesh = M.dmplex_like_numbering(M.structured_tri_mesh(9, 15, 1.0), seed=33)
    case = CS.dam_break_case(mesh, 1e9, dt=1e-3, perturb=0.0)
    case.u_local[:, 0] = 10.0
    c = interior_courant_numbers(case)
    assert int((c == np.nanmax(c)).sum()) >= 100
    op = CS.create_operator(case)
    u = _dev(case.u_local)
    for step in (False, True):
        if step:
            op.euler_step(case.dt, u, _dev(case.u_local))
        else:
            op.rhs_function(case.dt, u, _f(mesh))
        got, want = _async(op), _blocking(op)
        assert got == want and want[1] >= 0
    op.destroy()


# ---- 2. the place in the stream ------------------------------------------------------------------------------------------------

def test_the_result_is_that_of_begins_place_in_the_stream():
    a, b = _two_states()
    op = CS.create_operator(a)
    ua, ub, f = _dev(a.u_local), _dev(b.u_local), _f(a.mesh)
    op.rhs_function(a.dt, ua, f)
    want_a = _blocking(op)
    op.rhs_function(b.dt, ub, f)
    want_b = _blocking(op)
    assert want_a != want_b and want_a[1] >= 0 and want_b[1] >= 0
    op.rhs_function(a.dt, ua, f)
    op.diagnostics_begin()
    op.rhs_function(b.dt, ub, f)
    op.reset_diagnostics()
    op.diagnostics_wait()
    assert _bits(op.get_diagnostics()) == want_a
    op.rhs_function(b.dt, ub, f)
    assert _blocking(op) == want_b
    op.destroy()


# ---- 3. the rule that resolves the ids is the one in force at begin --------------------------------------------------------------

def test_the_owned_side_rule_is_captured_at_begin():
    op, case, u, g, o = _ghost_rank_operator()
    mesh = case.mesh
    swe_u = u[:, :3].contiguous()
    ghost, owned = int(mesh.cell_global_ids[g]), int(mesh.cell_global_ids[o])
    # each kind alone, with the blocking call: the two rules name different cells for this state
    op.rhs_function(case.dt, swe_u, _f(mesh))
    swe = _blocking(op)
    op.tracers_rhs_function(case.dt, u, _f(mesh, 5))
    tracers = _blocking(op)
    print(f"SWE rule {swe}, owned-side rule {tracers}; ghost cell {ghost}, owned cell {owned}")
    assert swe[2] == ghost and tracers[2] == owned and ghost != owned
    assert mesh.cell_is_owned[g] == 0 and mesh.cell_is_owned[o] != 0
    op.rhs_function(case.dt, swe_u, _f(mesh))
    op.diagnostics_begin()
    op.tracers_rhs_function(case.dt, u, _f(mesh, 5))     # flips the operator's flag while the read is out
    op.diagnostics_wait()
    assert _bits(op.get_diagnostics()) == swe
    # ... and the other way round
    op.tracers_rhs_function(case.dt, u, _f(mesh, 5))
    op.diagnostics_begin()
    op.rhs_function(case.dt, swe_u, _f(mesh))
    op.diagnostics_wait()
    assert _bits(op.get_diagnostics()) == tracers
    op.destroy()


# ---- 4. begin does not block ---------------------------------------------------------------------------------------------------

class _Filler:
    """A finite amount of device work of known duration on a stream of its own: repeated fills of a 1 GiB tensor, as many as its
    own event timing says make 40 ms (the tests ask for 20)."""

    def __init__(self):
        torch = _torch()
        self.stream = torch.cuda.Stream()
        self.big = torch.empty(1 << 27, dtype=torch.float64, device="cuda")
        self.count = 0
        ms = self.run(20)                  # (the first fills also pay for loading the kernel)
        ms = self.run(20)
        self.stream.synchronize()
        self.count = max(20, int(np.ceil(40.0 / (ms() / 20))))
        assert self.count <= 20000, self.count

    def run(self, n=None):
        """enqueues the fills; returns a function that gives their device time in ms once they have finished"""
        torch = _torch()
        start, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            start.record()
            for i in range(n or self.count):
                self.big.fill_(float(i))
            self.end.record()

        def ms():
            self.end.synchronize()
            return start.elapsed_time(self.end)
        return ms

    def hold_back(self, stream):
        """`stream` runs nothing more until the fills enqueued last have finished"""
        stream.wait_event(self.end)


def test_begin_returns_while_the_stream_is_held_back():
    torch = _torch()
    case, _ = _two_states()
    op = CS.create_operator(case)
    u, f = _dev(case.u_local), _f(case.mesh)
    op.rhs_function(case.dt, u, f)
    want = _blocking(op)
    op.rhs_function(case.dt, u, f)
    assert _async(op) == want              # the first begin of the scope allocates: only that one may synchronise
    filler = _Filler()
    torch.cuda.synchronize()
    ms = filler.run()
    filler.hold_back(torch.cuda.current_stream())
    op.rhs_function(case.dt, u, f)
    t0 = time.perf_counter()
    op.diagnostics_begin()
    begin_ms = 1e3 * (time.perf_counter() - t0)
    ready_right_after = op.diagnostics_ready()
    op.diagnostics_wait()
    ready_after_wait = op.diagnostics_ready()
    filler_ms = ms()
    print(f"filler: {filler.count} fills, {filler_ms:.2f} ms of device time; begin returned after {begin_ms:.3f} ms")
    assert filler_ms >= 20.0
    assert begin_ms < 0.5 * filler_ms       # a call that waits for the stream takes all of it
    assert ready_right_after is False and ready_after_wait is True
    assert _bits(op.get_diagnostics()) == want
    op.destroy()


# ---- 5. the state machine ------------------------------------------------------------------------------------------------------

def test_waits_with_nothing_in_flight_are_user_errors():
    case, _ = _two_states()
    op = CS.create_operator(case)
    assert _code(op.diagnostics_wait) == 83 and _code(op.diagnostics_ready) == 83        # no begin yet
    op.rhs_function(case.dt, _dev(case.u_local), _f(case.mesh))
    op.diagnostics_begin()
    op.diagnostics_wait()
    assert _code(op.diagnostics_wait) == 83                                            # already waited for
    assert "rdyhip_diagnostics_begin" in _lib.load().rdyhip_last_error().decode()
    op.destroy()


def test_a_second_begin_replaces_the_first():
    a, b = _two_states()
    op = CS.create_operator(a)
    ua, ub, f = _dev(a.u_local), _dev(b.u_local), _f(a.mesh)
    op.rhs_function(b.dt, ub, f)
    want_b = _blocking(op)
    op.rhs_function(a.dt, ua, f)
    op.diagnostics_begin()
    op.rhs_function(b.dt, ub, f)
    op.diagnostics_begin()
    op.diagnostics_wait()
    assert _bits(op.get_diagnostics()) == want_b
    assert _code(op.diagnostics_wait) == 83                                            # one read, one wait
    op.destroy()


def test_a_begin_on_another_stream_runs_behind_the_first_copy():
    """The first begin sits behind a held-back evaluation on stream 1; the second, on stream 2 and with nothing else ordering it,
    must see that evaluation's buckets -- its merge launch waits for the first copy.  Unordered, it would run at once and
    merge the empty buckets the reset left."""
    torch = _torch()
    case, _ = _two_states()
    op = CS.create_operator(case)
    u, f = _dev(case.u_local), _f(case.mesh)
    op.rhs_function(case.dt, u, f)
    want = _blocking(op)
    assert _async(op) == want and want[1] >= 0
    op.reset_diagnostics()
    filler = _Filler()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ms = filler.run()
    filler.hold_back(s1)
    with torch.cuda.stream(s1):
        op.rhs_function(case.dt, u, f)
        op.diagnostics_begin()
    with torch.cuda.stream(s2):
        op.diagnostics_begin()
    op.diagnostics_wait()
    assert _bits(op.get_diagnostics()) == want
    assert ms() >= 20.0
    torch.cuda.synchronize()
    op.destroy()


def test_the_blocking_call_discards_a_read_in_flight():
    a, b = _two_states()
    op = CS.create_operator(a)
    ua, ub, f = _dev(a.u_local), _dev(b.u_local), _f(a.mesh)
    op.rhs_function(b.dt, ub, f)
    want_b = _blocking(op)
    op.rhs_function(a.dt, ua, f)
    op.diagnostics_begin()
    op.rhs_function(b.dt, ub, f)
    assert _blocking(op) == want_b
    assert _code(op.diagnostics_wait) == 83
    assert _bits(op.get_diagnostics()) == want_b                                       # the blocking call's result stands
    op.destroy()


def test_destroy_with_a_read_in_flight():
    case, _ = _two_states()
    op = CS.create_operator(case)
    op.rhs_function(case.dt, _dev(case.u_local), _f(case.mesh))
    op.diagnostics_begin()
    op.destroy()


def test_scopes_that_cannot_be_read():
    case, _ = _two_states()
    op = CS.create_operator(case)
    lib = _lib.load()
    assert _code(op.ensemble_diagnostics_begin) == 83                                  # the ensemble scope before enable
    assert "not enabled" in lib.rdyhip_last_error().decode()
    assert _code(op.ensemble_diagnostics_wait) == 83
    for scope in (-1, 2, 7):
        assert lib.rdyhip_diagnostics_begin(op._h, scope, None) == 83 and b"scope" in lib.rdyhip_last_error()
        assert lib.rdyhip_diagnostics_wait(op._h, scope) == 83
    op.destroy()


def test_a_rank_that_owns_nothing():
    torch = _torch()
    mesh = _empty_mesh()
    op = Operator.create(RDyFlowConfig(), mesh)
    u = torch.zeros((mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    op.rhs_function(0.1, u, torch.empty((0, 3), dtype=torch.float64, device="cuda"))
    assert _async(op) == _bits_of(EMPTY) == _blocking(op)
    op.enable_ensemble(3)
    op.ensemble_rhs_function([0.1, 0.2, 0.3], torch.zeros((3, mesh.num_cells, 3), dtype=torch.float64, device="cuda"),
                             torch.empty((3, 0, 3), dtype=torch.float64, device="cuda"))
    op.ensemble_diagnostics_begin()
    op.ensemble_diagnostics_wait()
    assert [_bits(d) for d in op.ensemble_get_diagnostics()] == [_bits_of(EMPTY)] * 3
    op.destroy()


def _bits_of(t):
    return struct.unpack("<q", struct.pack("<d", t[0]))[0], t[1], t[2]


# ---- 6. the ensemble scope -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("tri-270", 3), ("tri-30", 64)])
def test_ensemble_scope_equals_the_blocking_call_for_every_member(name, B):
    torch = _torch()
    mesh = _mesh(name)
    cfg = RDyFlowConfig()
    cases = [random_case(np.random.default_rng(5200 + m), mesh, cfg) for m in range(B)]
    op = Operator.create(cfg, mesh, cases[0].condition_types)
    op.enable_ensemble(B)
    for m, case in enumerate(cases):
        assert case.condition_types == cases[0].condition_types
        _set_member(op, m, case)
    u = _dev(np.stack([c.u_local for c in cases]))
    f = torch.empty((B, mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.ensemble_rhs_function([c.dt for c in cases], u, f)
    op.ensemble_diagnostics_begin()
    op.ensemble_diagnostics_wait()
    got = [_bits(d) for d in op.ensemble_get_diagnostics()]
    op.ensemble_update_diagnostics()
    want = [_bits(d) for d in op.ensemble_get_diagnostics()]
    assert len(want) == B and got == want
    assert sum(w[1] >= 0 for w in want) >= B - 1 and len(set(want)) >= min(B, 3)        # real structs, the members' own
    assert _code(op.ensemble_diagnostics_wait) == 83
    # the two scopes are independent: the operator's own scope has nothing in flight
    assert _code(op.diagnostics_wait) == 83
    op.destroy()


# ---- 7. the stepper ------------------------------------------------------------------------------------------------------------

class _Rain:
    """the water source of interval k from a host array: the base rain times 1 + 0.5 (k mod 3)"""

    def __init__(self, op, base, interval):
        self.op, self.base, self.interval = op, base, interval

    def apply(self, time):
        k = int(round(time / self.interval))
        self.op.set_domain_external_source(0, self.base * (1.0 + 0.5 * (k % 3)), ordered=True)


def _ex2b_with_rain():
    case = CS.ex2b_case(os.path.join(GOLDEN, "planar_dam_10x5.msh"))
    case.ext_src[:, 0] = 1e-2 * (1.0 + 0.2 * np.sin(np.arange(case.mesh.num_owned_cells)))
    return case


@pytest.mark.parametrize("temporal", ["euler", "rk4"])
def test_pipelined_stepper_takes_the_same_steps_to_the_same_bits(temporal):
    torch = _torch()
    case = _ex2b_with_rain()
    runs = {}
    for pipelined in (False, True):
        op = CS.create_operator(case)
        st = EulerStepper(op, adaptive=AdaptiveTime(0.5, 2.0), forcing=_Rain(op, case.ext_src[:, 0].copy(), 0.2), temporal=temporal,
                          pipelined=pipelined)
        u = _dev(case.u_local)
        dt, dts, steps = 0.002, [], []
        for _ in range(10):
            dt = st.advance(u, dt, 0.2)
            dts.append(dt)
            steps.append(st.step)
        st.finish()
        torch.cuda.synchronize()
        runs[pipelined] = (dts, steps, u.clone(), st.max_courant, _bits(st.courant))
        op.destroy()
    (dts, steps, u0, c0, s0), (dts_p, steps_p, u1, c1, s1) = runs[False], runs[True]
    print(f"{temporal}: dt {dts}, steps {steps}")
    assert dts_p == dts and steps_p == steps and c1 == c0 and s1 == s0
    assert torch.equal(u1, u0)
    assert len(set(dts)) > 3 and steps[-1] > 20 and not torch.equal(u0, _dev(case.u_local))     # the rule has acted, the state has moved


# ---- 8. the C host -------------------------------------------------------------------------------------------------------------

def test_c_host_pipelined_against_blocking(tmp_path):
    case = _ex2b_with_rain()
    no = case.mesh.num_owned_cells
    path = str(tmp_path / "ex2b.bin")
    write_case(path, case, True, np.zeros((no, 3)), np.zeros((no, 3)), np.zeros((no, 3)), 0.0)
    args = ["12", repr(0.2), repr(0.002), "1", repr(0.4), repr(1.5)]
    env = dict(os.environ)
    env.pop("RDYHIP_LIB", None)

    def run(exe, tag, extra):
        out = str(tmp_path / f"{tag}.bin")
        r = subprocess.run([exe, path, out] + args + extra, capture_output=True, text=True, env=env, timeout=120)
        print(tag, r.stdout, r.stderr)
        assert r.returncode == 0, (tag, r.returncode, r.stdout, r.stderr)
        return open(out, "rb").read()
    pipe, adv = compile_client(tmp_path, "rdyhip_pipeline_client"), compile_client(tmp_path, "rdyhip_advance_client")
    vary = {p: run(pipe, f"p{p}v1", [str(p), "1"]) for p in (0, 1)}
    assert vary[1] == vary[0]
    same = {p: run(pipe, f"p{p}v0", [str(p), "0"]) for p in (0, 1)}
    reference = run(adv, "advance", [])
    assert same[0] == reference and same[1] == reference
    assert vary[0] != reference                                                        # the refreshed rain is felt
    assert struct.unpack("q", reference[:8])[0] > 100 and len(reference) == 24 + 8 * 3 * case.mesh.num_cells
