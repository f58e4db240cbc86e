"""GPU: the time series kept on the device (rdyhip_series_*, csrc/series_kernels.h) against the loop they replace -- a host that
reads the accumulated fluxes of every boundary back through rdyhip_get_boundary_fluxes after a step, forms
(edge length * flux) / accumulated time in numpy and calls rdyhip_reset_boundary_fluxes_accum -- bit for bit, and against
the oracle's own boundary_fluxes_accum.

Meshes, states and step sizes: those of tests/test_gpu_output_mean.py (its docstring says why they stay finite for three
steps): tri-prefix, quad-prefix, tri-o2l (the owned index is not the local one; 1 boundary edge behind a ghost cell) and
quad-odd (567 owned quads, 21 ghosts; 23 of its 98 boundary edges behind a ghost cell).  All three condition types occur.
An edge that is dry on both sides holds NaN in its accumulator (tests/test_gpu_conservation.py), and the record keeps it: the
comparisons are "the same 64 bits where the reference is finite, NaN where it is NaN", and every case must hold both kinds
of entries or the comparison would be vacuous.  With the CPU oracle after the three steps, NaN / finite non-zero water fluxes
on the edges a record holds: 28/80, 36/113, 4/24, 20/55 for the four meshes (first order; similar with HR).

The monitor the tests play around the steps is WriteTimeSeries (src/time_series.c:530-564): at step 0 and after every step,
observations if step % interval == 0, then add_time(dt of the step; at step 0 the first step's), then the boundary record if
step % interval == 0.
Tolerance against the oracle: TOL of test_gpu_parity.py, rel L-inf against max(1, |ref|) on the finite entries.
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
from rdycore_amd.operator import (SERIES_BOUNDARY_FLUXES, SERIES_OBSERVATIONS, SOURCE_SEMI_IMPLICIT, Operator, RDyFlowConfig,
                                  plan_series_boundary_edges)

from helpers import oracle_from_case, rel_linf
from test_gpu_c_client import compile_client, write_case
from test_gpu_output_mean import DTS, MESHES, PATHS, _case, _dev, _interval_steps, _skip_hr_behind_the_cell_kernel, _torch
from test_gpu_parity import TOL, tri_mms_case

pytestmark = pytest.mark.gpu

DTS4 = DTS + (2e-4,)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sites(case, n=40, seed=5):
    """owned-cell indices drawn by a seeded generator, some of them twice"""
    rng = np.random.default_rng(seed + case.mesh.num_owned_cells)
    s = rng.integers(0, case.mesh.num_owned_cells, size=n).astype(np.int32)
    s[n // 2] = s[3]
    s[-1] = s[0]
    assert np.unique(s).size < n
    return s


def _listed(case, which):
    """all boundaries, or all but the last in descending order (the order of the list must not matter)"""
    nb = len(case.mesh.boundaries)
    return None if which == "all" else list(range(nb - 1))[::-1]


class Rows:
    """the rows of a record, restated: for the listed boundaries in ascending index, the positions inside the boundary of the
    edges whose left cell is owned, and their lengths"""

    def __init__(self, mesh, listed):
        left = np.asarray(mesh.edge_cell_ids).reshape(-1, 2)[:, 0]
        owned = np.asarray(mesh.cell_is_owned)
        self.mesh = mesh
        self.per_boundary = []
        for b, boundary in enumerate(mesh.boundaries):
            if listed is not None and b not in listed:
                continue
            e = np.asarray(boundary.edge_ids)
            keep = np.nonzero(owned[left[e]])[0]
            self.per_boundary.append((b, keep, e[keep]))
        self.edges = np.concatenate([e for _, _, e in self.per_boundary] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
        self.E = int(self.edges.size)

    def record(self, accum_of, T):
        """(len[:, None] * acc) / T on the owned-left edges: RecordBoundaryFluxes' product, WriteBoundaryFluxes' division"""
        out = [np.zeros((0, 3))]
        with np.errstate(invalid="ignore"):
            for b, keep, e in self.per_boundary:
                acc = accum_of(b)
                out.append(((np.asarray(self.mesh.edge_lengths)[e][:, None] * acc[keep]) / T))
        return np.concatenate(out)


class HostLoop:
    """the parent's way: after a step, one blocking read per boundary, the arithmetic in numpy, one blocking reset"""

    def __init__(self, op, case, sites, listed, interval):
        self.op, self.case, self.interval = op, case, interval
        self.rows = Rows(case.mesh, listed)
        self.own = np.asarray(case.mesh.cell_owned_to_local)
        self.sites = sites
        self.T = 0.0
        self.flux, self.obs, self.flux_times, self.obs_times = [], [], [], []

    def monitor(self, step, time, dt, u):
        if step % self.interval == 0:
            self.obs.append(u.cpu().numpy()[self.own[self.sites]])
            self.obs_times.append(time)
        self.T += dt
        if step % self.interval == 0:
            T = 1.0 if self.T == 0.0 else self.T
            acc = [self.op.boundary_fluxes(b, accumulated=True) for b in range(len(self.case.mesh.boundaries))]
            self.flux.append(self.rows.record(lambda b: acc[b], T))
            self.flux_times.append(time)
            self.op.reset_boundary_fluxes_accum()
            self.T = 0.0

    def result(self):
        return (np.array(self.flux_times), np.array(self.flux).reshape(-1, self.rows.E, 3),
                np.array(self.obs_times), np.array(self.obs).reshape(-1, self.sites.size, 3))


class NewCalls:
    """the records on the device; after every boundary record the accumulators of EVERY boundary must read back +0.0"""

    def __init__(self, op, case, sites, listed, interval, capacity=8):
        self.op, self.case, self.interval = op, case, interval
        op.enable_observation_series(sites, capacity)
        op.enable_boundary_flux_series(capacity, listed)

    def monitor(self, step, time, dt, u):
        if step % self.interval == 0:
            self.op.series_record(SERIES_OBSERVATIONS, time, u)
        self.op.series_add_time(dt)
        if step % self.interval == 0:
            self.op.series_record(SERIES_BOUNDARY_FLUXES, time)
            for b in range(len(self.case.mesh.boundaries)):
                acc = self.op.boundary_fluxes(b, accumulated=True)
                assert not _bits(acc).any(), f"boundary {b}: accumulators are not +0.0 after the record of step {step}"
            assert self.op.series_info(SERIES_BOUNDARY_FLUXES)["accumulated_time"] == 0.0

    def result(self):
        ft, fv = self.op.series_read(SERIES_BOUNDARY_FLUXES)
        ot, ov = self.op.series_read(SERIES_OBSERVATIONS)
        return ft, fv, ot, ov


def _run_steps(op, case, path, dts, series):
    """the steps of `path` with the monitor's calls around them; the state after the last step and what `series` kept"""
    torch = _torch()
    no = case.mesh.num_owned_cells
    u = _dev(case.u_local)
    u2 = u.clone()
    f = torch.empty((no, 3), dtype=torch.float64, device="cuda")
    time = 0.0
    series.monitor(0, time, dts[0], u)
    for k, dt in enumerate(dts):
        if path == "euler_fused":
            op.euler_step(dt, u, u2)
            u, u2 = u2, u
        elif path == "rhs_axpy":
            op.rhs_function(dt, u, f)
            op.axpy_owned(dt, f, u)
        else:
            op.rk4_step(dt, u)
        time += dt
        series.monitor(k + 1, time, dt, u)
    out = series.result()
    torch.cuda.synchronize()
    return u.cpu().numpy(), out


@functools.lru_cache(maxsize=None)
def _new_path_run(name, hr, path, interval, kernel):
    """the new calls, once per (mesh, order, path, interval, kernel variant -- the fixture has set it); shared by the tests"""
    assert os.environ.get("RDYHIP_KERNEL") == kernel
    case = _case(name, hr)
    which = "all" if interval == 1 else "subset"
    dts = DTS if interval == 1 else DTS4
    op = CS.create_operator(case)
    u, out = _run_steps(op, case, path, dts, NewCalls(op, case, _sites(case), _listed(case, which), interval))
    edges = op.series_boundary_edges()
    op.destroy()
    return u, out, edges


def _assert_same_records(got, ref, what, need_nan=True):
    """finite entries: the same 64 bits; NaN entries: NaN at the same positions; both kinds present"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    assert not np.isinf(ref).any() and not np.isinf(got).any(), what
    assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan]), f"{what}: {int((_bits(got)[~nan] != _bits(ref)[~nan]).sum())} finite entries differ in their bits"
    nonzero = int((~nan & (ref != 0.0)).sum())
    print(f"{what}: {int(nan.sum())} NaN, {nonzero} finite non-zero of {ref.size} entries")
    assert nonzero > 0 and (nan.any() or not need_nan), f"{what}: the comparison is vacuous"


# ---- 1. the bits of the loop it replaces ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("interval", [1, 2])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
@pytest.mark.parametrize("name", MESHES)
def test_records_are_the_bits_of_the_host_loop(name, hr, path, interval, rdyhip_kernel):
    """interval 1: three steps, four records, every boundary listed; interval 2: four steps, three records, the last boundary
    left out (its accumulators are reset all the same, NewCalls asserts it)"""
    _skip_hr_behind_the_cell_kernel(hr, rdyhip_kernel)
    case = _case(name, hr)
    what = f"{name}-{'hr' if hr else 'plain'}-{path}-every-{interval}"
    which = "all" if interval == 1 else "subset"
    dts = DTS if interval == 1 else DTS4
    sites = _sites(case)
    a = CS.create_operator(case)
    host = HostLoop(a, case, sites, _listed(case, which), interval)
    ua, (ft_a, fv_a, ot_a, ov_a) = _run_steps(a, case, path, dts, host)
    a.destroy()
    ub, (ft_b, fv_b, ot_b, ov_b), (edges, bnds) = _new_path_run(name, hr, path, interval, rdyhip_kernel)
    nrec = 4 if interval == 1 else 3
    assert fv_b.shape == (nrec, host.rows.E, 3) and ov_b.shape == (nrec, 40, 3) and host.rows.E > 0
    assert np.array_equal(edges, host.rows.edges)
    assert np.array_equal(ft_a, ft_b) and np.array_equal(ot_a, ot_b) and ft_b[0] == 0.0 and abs(ft_b[-1] - sum(dts)) <= 1e-15
    _assert_same_records(fv_b, fv_a, what)
    assert not _bits(fv_b[0]).any(), "the record at step 0 is not +0.0 everywhere"
    # the observations: u[o2l[sites]] after every step, bit for bit; and the two operators took the same steps
    assert np.isfinite(ov_a).all() and np.array_equal(_bits(ov_b), _bits(ov_a)), f"{what}: observations"
    assert np.array_equal(_bits(ov_b[-1]), _bits(ub[np.asarray(case.mesh.cell_owned_to_local)[sites]]))
    assert np.array_equal(_bits(ua), _bits(ub)), f"{what}: final state"
    if name == "tri-o2l":
        assert not np.array_equal(np.asarray(case.mesh.cell_owned_to_local)[sites], sites)
    assert set(case.condition_types) == {0, 2, 3}                              # Dirichlet, reflecting, critical outflow


# ---- 2. more than one workgroup ------------------------------------------------------------------------------------------------

def test_more_than_one_workgroup(rdyhip_kernel):
    """12 000 triangles, K = 320 boundary edges: two workgroups of the record kernel, the second partial; 300 sites: two of the
    observation kernel's.  Four Euler steps of 1 - 2 ms."""
    case = tri_mms_case(100, 60, SOURCE_SEMI_IMPLICIT, order="tiled")
    assert case.mesh.num_owned_cells == 12000 and sum(b.num_edges for b in case.mesh.boundaries) == 320
    dts = (1e-3, 2e-3, 1.5e-3, 1e-3)
    sites = _sites(case, n=300)
    a = CS.create_operator(case)
    host = HostLoop(a, case, sites, None, 1)
    ua, (ft_a, fv_a, ot_a, ov_a) = _run_steps(a, case, "euler_fused", dts, host)
    a.destroy()
    b = CS.create_operator(case)
    ub, (ft_b, fv_b, ot_b, ov_b) = _run_steps(b, case, "euler_fused", dts, NewCalls(b, case, sites, None, 1))
    b.destroy()
    assert fv_b.shape == (5, 320, 3) and ov_b.shape == (5, 300, 3)
    assert np.array_equal(ft_a, ft_b) and np.array_equal(ot_a, ot_b)
    _assert_same_records(fv_b, fv_a, "tri 100 x 60")
    assert np.isfinite(ov_a).all() and np.array_equal(_bits(ov_b), _bits(ov_a)) and np.array_equal(_bits(ua), _bits(ub))


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_records(name, hr, path):
    case = _case(name, hr)
    orc = oracle_from_case(case)
    own = np.asarray(case.mesh.cell_owned_to_local)
    rows = Rows(case.mesh, None)
    u = case.u_local.copy()

    def rhs(dt, state):
        orc.reset_diagnostics()
        return orc.apply(dt, state)

    def record(T):
        rec = rows.record(lambda b: orc.boundary_fluxes_accum[b], T).copy()
        for acc in orc.boundary_fluxes_accum:
            acc[:] = 0.0
        return rec
    records = [record(DTS[0])]
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
        records.append(record(dt))
    return u, np.array(records)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
@pytest.mark.parametrize("name", MESHES)
def test_records_match_the_oracle(name, hr, path, rdyhip_kernel):
    _torch()
    _skip_hr_behind_the_cell_kernel(hr, rdyhip_kernel)
    _, (ft, fv, ot, ov), _ = _new_path_run(name, hr, path, 1, rdyhip_kernel)
    u_ref, ref = _oracle_records(name, hr, path)
    assert np.isfinite(u_ref).all(), "the oracle loop left the finite numbers: the test's states are not fit for three steps"
    assert fv.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(fv), nan), "NaN positions differ from the oracle's"
    err = rel_linf(fv[~nan], ref[~nan])
    print(f"{name}-{'hr' if hr else 'plain'}-{path}: rel L-inf {err:.3e}, {int(nan.sum())} NaN, {int((~nan & (ref != 0)).sum())} finite non-zero")
    assert err <= TOL, f"records: rel L-inf {err:.3e}"
    assert nan.any() and (~nan & (ref != 0.0)).any()
    # Runge-Kutta: every stage has added its dt x flux, a record holds about four times an Euler step's
    case = _case(name, hr)
    assert rel_linf(ov[-1], u_ref[np.asarray(case.mesh.cell_owned_to_local)[_sites(case)]]) <= TOL


# ---- 4. ranks ------------------------------------------------------------------------------------------------------------------

def _rank_cases(kind, world):
    if kind == "quads":
        g = CS.dam_break_quads_case(CS.dam_break_quads_mesh(96, 48))
        parts = [CS.dam_break_quads_case(CS.dam_break_quads_mesh(96, 48, r, world)) for r in range(world)]
        xc, yc = g.mesh.cell_centroids[:, 0], g.mesh.cell_centroids[:, 1]       # a moving state, as tests/test_gpu_multirank.py
        g.u_local[:, 0] *= 1.0 + 1e-3 * xc / 10.0 + 2e-3 * yc / 5.0
        g.u_local[:, 1] = 0.3 * g.u_local[:, 0] * np.sin(1.7 * xc + 0.9 * yc)
        g.u_local[:, 2] = 0.2 * g.u_local[:, 0] * np.cos(1.1 * xc - 2.3 * yc)
    else:
        g = CS.c5_case(CS.c5_mesh(60, 50), 60.0, 50.0)
        parts = [CS.c5_case(CS.c5_mesh(60, 50, r, world), 60.0, 50.0) for r in range(world)]
    return g, parts


@pytest.mark.parametrize("kind", ["quads", "c5"])
def test_three_ranks_record_what_one_rank_records(kind, rdyhip_kernel):
    """one structured mesh cut into 3 parts (partitioned_structured_mesh), the parts one after the other on the one device,
    ghosts filled from the global state: the union of the three records, keyed by global edge id, is the undivided mesh's"""
    torch = _torch()
    _skip_hr_behind_the_cell_kernel(kind == "c5", rdyhip_kernel)
    g, parts = _rank_cases(kind, 3)
    dt = g.dt
    g2row = {int(gid): i for i, gid in enumerate(g.mesh.cell_global_ids)}

    def one(case, u_host):
        op = CS.create_operator(case)
        op.enable_boundary_flux_series(2)
        u = _dev(u_host)
        f = torch.empty((case.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
        op.rhs_function(dt, u, f)
        op.series_add_time(dt)
        op.series_record(SERIES_BOUNDARY_FLUXES, dt)
        _, rec = op.series_read(SERIES_BOUNDARY_FLUXES)
        edges, bnds = op.series_boundary_edges()
        op.destroy()
        gids = np.asarray(case.mesh.edge_global_ids)[edges]
        assert np.unique(gids).size == gids.size
        return {int(e): (int(b), rec[0, i]) for i, (e, b) in enumerate(zip(gids, bnds))}

    whole = one(g, g.u_local)
    all_boundary_edges = np.concatenate([np.asarray(g.mesh.edge_global_ids)[np.asarray(b.edge_ids)] for b in g.mesh.boundaries])
    assert sorted(whole) == sorted(int(e) for e in all_boundary_edges)
    union, ghost_left = {}, 0
    for case in parts:
        m = case.mesh
        u_part = g.u_local[[g2row[int(gid)] for gid in m.cell_global_ids]]      # owned and ghost rows from the global state
        mine = one(case, u_part)
        assert mine and not (set(mine) & set(union)), "a boundary edge is recorded by two ranks"
        union.update(mine)
        left = np.asarray(m.edge_cell_ids).reshape(-1, 2)[:, 0]
        ghost_left += sum(int((np.asarray(m.cell_is_owned)[left[np.asarray(b.edge_ids)]] == 0).sum()) for b in m.boundaries)
    assert sorted(union) == sorted(whole), "the ranks' records do not cover every global boundary edge exactly once"
    got = np.array([union[e][1] for e in sorted(whole)])
    ref = np.array([whole[e][1] for e in sorted(whole)])
    assert [union[e][0] for e in sorted(whole)] == [whole[e][0] for e in sorted(whole)]
    _assert_same_records(got, ref, f"3 ranks, {kind}", need_nan=False)
    print(f"{kind}: {len(whole)} boundary edges, {ghost_left} of the parts' boundary edges lie behind ghost cells")


# ---- 5. windows and errors -----------------------------------------------------------------------------------------------------

def _raises_user_error(call):
    with pytest.raises(RDyHipError) as e:
        call()
    assert e.value.code == 83, e.value
    return e.value


def _accumulators(op, case):
    return [op.boundary_fluxes(b, accumulated=True) for b in range(len(case.mesh.boundaries))]


def test_windows_full_log_clear_and_sub_range_reads(rdyhip_kernel):
    torch = _torch()
    case = _case("quad-odd", False)
    no, K = case.mesh.num_owned_cells, sum(b.num_edges for b in case.mesh.boundaries)
    sites = _sites(case, n=7)
    rows = Rows(case.mesh, None)
    op = CS.create_operator(case)
    b0 = op.layout_info()["device_bytes"]
    op.enable_observation_series(sites, 3)
    assert op.layout_info()["device_bytes"] - b0 == 3 * 7 * 24 + 7 * 4
    b1 = op.layout_info()["device_bytes"]
    op.enable_boundary_flux_series(3)
    assert op.layout_info()["device_bytes"] - b1 == 3 * rows.E * 24 + K * 4 + K * 8 and rows.E == 75 and K == 98
    assert op.series_info(SERIES_BOUNDARY_FLUXES) == {"entries": 75, "count": 0, "capacity": 3, "accumulated_time": 0.0}
    assert op.series_info(SERIES_OBSERVATIONS) == {"entries": 7, "count": 0, "capacity": 3, "accumulated_time": 0.0}
    u = _dev(case.u_local)
    f = torch.empty((no, 3), dtype=torch.float64, device="cuda")
    # a record with accumulated time 0 divides by 1
    op.rhs_function(DTS[0], u, f)
    acc = _accumulators(op, case)
    op.series_record(SERIES_BOUNDARY_FLUXES, 0.5)
    expect = [rows.record(lambda b: acc[b], 1.0)]
    # two more with a time
    for k, dt in enumerate(DTS[1:]):
        op.rhs_function(dt, u, f)
        op.series_add_time(dt)
        op.series_add_time(dt)
        acc = _accumulators(op, case)
        assert op.series_info(SERIES_BOUNDARY_FLUXES)["accumulated_time"] == dt + dt
        op.series_record(SERIES_BOUNDARY_FLUXES, 1.0 + k)
        op.series_record(SERIES_OBSERVATIONS, 1.0 + k, u)
        expect.append(rows.record(lambda b: acc[b], dt + dt))
    # the log is full: 83, and neither the accumulators nor the times change
    op.rhs_function(DTS[0], u, f)
    op.series_add_time(0.125)
    acc = _accumulators(op, case)
    err = _raises_user_error(lambda: op.series_record(SERIES_BOUNDARY_FLUXES, 9.0))
    assert "full" in err.message
    after = _accumulators(op, case)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(acc, after)) and any(_bits(x).any() for x in after)
    assert op.series_info(SERIES_BOUNDARY_FLUXES) == {"entries": 75, "count": 3, "capacity": 3, "accumulated_time": 0.125}
    times, values = op.series_read(SERIES_BOUNDARY_FLUXES)
    assert times.tolist() == [0.5, 1.0, 2.0]
    _assert_same_records(values, np.array(expect), "three windows")
    # a sub-range: the right rows and times; a range outside the log: 83
    t1, v1 = op.series_read(SERIES_BOUNDARY_FLUXES, first=1, count=2)
    assert t1.tolist() == [1.0, 2.0] and np.array_equal(_bits(v1)[~np.isnan(v1)], _bits(values[1:])[~np.isnan(v1)])
    t2, v2 = op.series_read(SERIES_OBSERVATIONS, first=1, count=1)
    assert t2.tolist() == [2.0] and np.array_equal(_bits(v2[0]), _bits(case.u_local[np.asarray(case.mesh.cell_owned_to_local)[sites]]))
    _raises_user_error(lambda: op.series_read(SERIES_BOUNDARY_FLUXES, first=2, count=2))
    _raises_user_error(lambda: op.series_read(SERIES_BOUNDARY_FLUXES, first=-1, count=1))
    # the log on the device, without a copy
    log = op.series_device_log(SERIES_BOUNDARY_FLUXES)
    assert tuple(log.shape) == (3, 75, 3) and np.array_equal(_bits(log.cpu().numpy())[~np.isnan(values)], _bits(values)[~np.isnan(values)])
    # clear makes room and leaves the accumulated time alone
    op.series_clear(SERIES_BOUNDARY_FLUXES)
    assert op.series_info(SERIES_BOUNDARY_FLUXES) == {"entries": 75, "count": 0, "capacity": 3, "accumulated_time": 0.125}
    assert op.series_info(SERIES_OBSERVATIONS)["count"] == 2
    op.series_record(SERIES_BOUNDARY_FLUXES, 3.0)
    times, values = op.series_read(SERIES_BOUNDARY_FLUXES)
    assert times.tolist() == [3.0]
    _assert_same_records(values, np.array([rows.record(lambda b: acc[b], 0.125)]), "after clear")
    assert not any(_bits(x).any() for x in _accumulators(op, case))
    op.destroy()


def test_argument_errors(rdyhip_kernel):
    case = _case("quad-odd", False)
    no, nb = case.mesh.num_owned_cells, len(case.mesh.boundaries)
    u = _dev(case.u_local)
    op = CS.create_operator(case)
    b0 = op.layout_info()["device_bytes"]
    # nothing is enabled yet
    for kind in (SERIES_OBSERVATIONS, SERIES_BOUNDARY_FLUXES):
        err = _raises_user_error(lambda: op.series_record(kind, 0.0, u))
        assert "not enabled" in err.message
        _raises_user_error(lambda: op.series_info(kind))
        _raises_user_error(lambda: op.series_read(kind, 0, 0))
        _raises_user_error(lambda: op.series_clear(kind))
        _raises_user_error(lambda: op.series_device_log(kind))
    _raises_user_error(lambda: op.series_add_time(0.1))
    _raises_user_error(op.series_boundary_edges)
    # a site or a boundary out of range, negative capacities: 83 and nothing is allocated
    _raises_user_error(lambda: op.enable_observation_series([0, no], 4))
    _raises_user_error(lambda: op.enable_observation_series([-1], 4))
    _raises_user_error(lambda: op.enable_observation_series([0], -1))
    _raises_user_error(lambda: op.enable_boundary_flux_series(4, [nb]))
    _raises_user_error(lambda: op.enable_boundary_flux_series(4, [0, -1]))
    _raises_user_error(lambda: op.enable_boundary_flux_series(-1))
    assert op.layout_info()["device_bytes"] == b0
    op.enable_observation_series([0, no - 1, 0], 4)
    op.enable_boundary_flux_series(4, [0])
    b1 = op.layout_info()["device_bytes"]
    # a second enable, an unknown kind, a missing state array
    assert "already" in _raises_user_error(lambda: op.enable_observation_series([1], 4)).message
    assert "already" in _raises_user_error(lambda: op.enable_boundary_flux_series(4)).message
    for kind in (0, 3, -1):
        assert "kind" in _raises_user_error(lambda: op.series_record(kind, 0.0, u)).message
        _raises_user_error(lambda: op.series_info(kind))
        _raises_user_error(lambda: op.series_clear(kind))
    _raises_user_error(lambda: op.series_record(SERIES_OBSERVATIONS, 0.0, None))
    assert op.layout_info()["device_bytes"] == b1
    assert op.series_info(SERIES_OBSERVATIONS)["count"] == 0 and op.series_info(SERIES_BOUNDARY_FLUXES)["count"] == 0
    edges, bnds = op.series_boundary_edges()
    ref_e, ref_b = plan_series_boundary_edges(case.mesh, [0])
    assert np.array_equal(edges, ref_e) and np.array_equal(bnds, ref_b) and edges.size == 21
    op.destroy()


def test_series_without_entries_advance_their_counts_and_launch_nothing(rdyhip_kernel):
    torch = _torch()
    # a rank that owns nothing
    xyz, conn, _, _ = M.structured_tri_connectivity(3, 2)
    mesh = M.build_mesh(xyz, conn, is_owned=np.zeros(conn.shape[0], dtype=np.int32), boundary_classifier=M.box_side_boundaries(0, 3, 0, 2))
    assert mesh.num_owned_cells == 0
    op = Operator.create(RDyFlowConfig(), mesh)
    u = torch.ones((mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    f = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    op.enable_observation_series([], 2)
    op.enable_boundary_flux_series(2)
    assert op.series_info(SERIES_BOUNDARY_FLUXES)["entries"] == 0 and op.series_info(SERIES_OBSERVATIONS)["entries"] == 0
    op.rhs_function(0.1, u, f)
    for k in range(2):
        op.series_record(SERIES_OBSERVATIONS, 0.25 * k, None)
        op.series_add_time(0.5)
        op.series_record(SERIES_BOUNDARY_FLUXES, 0.25 * k)
    _raises_user_error(lambda: op.series_record(SERIES_BOUNDARY_FLUXES, 1.0))
    for kind in (SERIES_OBSERVATIONS, SERIES_BOUNDARY_FLUXES):
        assert op.series_info(kind) == {"entries": 0, "count": 2, "capacity": 2, "accumulated_time": 0.0}
        times, values = op.series_read(kind)
        assert times.tolist() == [0.0, 0.25] and values.shape == (2, 0, 3)
        assert tuple(op.series_device_log(kind).shape) == (2, 0, 3)
    e, b = op.series_boundary_edges()
    assert e.size == 0 and b.size == 0
    torch.cuda.synchronize()
    op.destroy()
    # an empty list on a rank with boundary edges: E == 0, so nothing is launched -- the accumulators keep what they hold
    case = _case("quad-odd", False)
    op = CS.create_operator(case)
    op.enable_boundary_flux_series(2, [])
    u = _dev(case.u_local)
    f = torch.empty((case.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.rhs_function(DTS[0], u, f)
    acc = _accumulators(op, case)
    op.series_add_time(DTS[0])
    op.series_record(SERIES_BOUNDARY_FLUXES, DTS[0])
    after = _accumulators(op, case)
    assert any(_bits(x).any() for x in acc) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(acc, after))
    assert op.series_info(SERIES_BOUNDARY_FLUXES) == {"entries": 0, "count": 1, "capacity": 2, "accumulated_time": 0.0}
    op.destroy()


# ---- 6. the stepper ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("temporal", ["euler", "rk4"])
def test_stepper_makes_the_explicit_call_sequence(temporal, rdyhip_kernel):
    torch = _torch()
    from rdycore_amd.timestep import EulerStepper, TimeSeries
    case = _case("quad-prefix", False)                         # no ghost cells: without a halo the stepper's second array has none to fill
    assert case.mesh.num_cells == case.mesh.num_owned_cells
    sites = _sites(case)
    dt, interval = 2e-4, 5e-4                                  # 0.2 + 0.2 + 0.1 ms: a shortened last step, its time added as 0.2 ms
    obs_every, flux_every = 2, 1
    a = CS.create_operator(case)
    ua = _dev(case.u_local)
    st = EulerStepper(a, temporal=temporal, series=TimeSeries(observation_sites=sites, observation_interval=obs_every,
                                                               boundary_flux_interval=flux_every, boundaries=[2, 0], capacity=16))
    # the explicit sequence
    b = CS.create_operator(case)
    b.enable_observation_series(sites, 16)
    b.enable_boundary_flux_series(16, [2, 0])
    ub = _dev(case.u_local)
    u2 = ub.clone()

    def monitor(step, time, state):
        if step % obs_every == 0:
            b.series_record(SERIES_OBSERVATIONS, time, state)
        b.series_add_time(dt)
        if step % flux_every == 0:
            b.series_record(SERIES_BOUNDARY_FLUXES, time)
    time, step = 0.0, 0
    monitor(0, 0.0, ub)
    for window in range(2):
        assert st.advance(ua, dt, interval) == dt
        hs, _ = _interval_steps(time, dt, interval)
        assert len(hs) == 3 and hs[2] < dt
        b.reset_diagnostics()
        cur, nxt = ub, u2
        for h in hs:
            if temporal == "rk4":
                b.rk4_step(h, ub)
            else:
                b.euler_step(h, cur, nxt)
                cur, nxt = nxt, cur
            time += h
            step += 1
            monitor(step, time, cur)
        if cur is not ub:
            ub.copy_(cur)
    assert st.step == 6 and abs(st.time - 1e-3) <= 1e-15 and st.time == time
    for kind, n in ((SERIES_OBSERVATIONS, 4), (SERIES_BOUNDARY_FLUXES, 7)):
        ta, va = st.series_read(kind)
        tb, vb = b.series_read(kind)
        assert ta.size == n and np.array_equal(ta, tb)
        nan = np.isnan(vb)
        assert np.array_equal(np.isnan(va), nan) and np.array_equal(_bits(va)[~nan], _bits(vb)[~nan]), f"records of series {kind}"
        assert (~nan & (vb != 0.0)).any()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ua.cpu().numpy()), _bits(ub.cpu().numpy()))
    assert a.series_info(SERIES_BOUNDARY_FLUXES)["accumulated_time"] == 0.0
    a.destroy()
    b.destroy()


# ---- 7. the C host -------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_c_host_keeps_the_series(tmp_path, rdyhip_kernel):
    """tests/c_client/rdyhip_series_client.c: the three fused Euler steps of tri-o2l (first order) with both series every step,
    from a case file whose trailer holds the sites, the listed boundaries and the records of test 1's new path"""
    _torch()
    build.build_native()
    case = _case("tri-o2l", False)
    _, (ft, fv, ot, ov), (edges, _) = _new_path_run("tri-o2l", False, "euler_fused", 1, rdyhip_kernel)
    sites = _sites(case)
    no = case.mesh.num_owned_cells
    path = str(tmp_path / "case.bin")
    write_case(path, case, True, np.zeros((no, 3)), np.zeros((no, 3)), np.zeros((no, 3)), 0.0)
    assert np.array_equal(ft, ot) and fv.shape[0] == len(DTS) + 1
    trailer = struct.pack("i", len(DTS)) + np.asarray(DTS, dtype=np.float64).tobytes()
    trailer += struct.pack("i", sites.size) + sites.astype(np.int32).tobytes()
    trailer += struct.pack("i", -1)                                           # every boundary
    trailer += struct.pack("i", edges.size) + ft.tobytes() + np.ascontiguousarray(fv).tobytes() + np.ascontiguousarray(ov).tobytes()
    with open(path, "ab") as fh:
        fh.write(trailer + struct.pack("q", len(trailer)))
    exe = compile_client(tmp_path, "rdyhip_series_client")
    env = dict(os.environ)
    env.pop("RDYHIP_LIB", None)
    run = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=100)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "records ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
    assert f"{len(DTS) + 1} records of {edges.size} boundary edges" in run.stdout and np.isnan(fv).any()
