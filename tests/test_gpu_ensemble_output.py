"""GPU: ensemble output (rdyhip_ens_state_* / _error_sums / _output_mean_* / _series_* / _stats, csrc/ens_output_kernels.h).  Every
call serves all B members in one launch, and every result is compared BIT FOR BIT with what the per-operator calls give on the
members' slices of the same [B, num_cells, 3] array (rdyhip_state_planes, rdyhip_error_sums, rdyhip_output_mean_*), with the rows
of the state itself (series), or with the numpy restatement of the statistics rule in test_ensemble_output_cpu.py: no tolerance
anywhere.  Meshes and members are those of test_gpu_ensemble.py and test_ensemble_hr_cpu.py: tri-30, quad-44, mixed and part-o2l
(972 owned cells of 1043, owned cells not a prefix: the smallest case with loc(o) != o) at B = 1, 3, 7 (the groups do not divide
it) and B = 64 on tri-30."""
import ctypes as C
import functools

import numpy as np
import pytest

from rdycore_amd import _lib
from rdycore_amd import mesh as M
from rdycore_amd.operator import (COMPONENT_H, COMPONENT_HU, COMPONENT_HV, OUTPUT_PRIMITIVE_VARIABLES, OUTPUT_SOLUTION, OUTPUT_SOURCES, Operator,
                                  RDyFlowConfig, RDyHipError, SOURCE_IMPLICIT_XQ2018, SOURCE_SEMI_IMPLICIT, WELL_BALANCING_HR)
from rdycore_amd.timestep import EnsembleEulerStepper, TimeSeries
from test_ensemble_hr_cpu import members as hr_members
from test_ensemble_output_cpu import ensemble_stats_rule, planted_rows
from test_gpu_ensemble import _bits, _dev, _members, _operator, _set_member, _torch
from test_gpu_tracers import _bathymetry, _empty_mesh

pytestmark = pytest.mark.gpu

SRC = SOURCE_SEMI_IMPLICIT
CONFIGS = [(name, B) for name in ("tri-30", "quad-44", "mixed", "part-o2l") for B in (1, 3, 7)] + [("tri-30", 64)]
VARS = (OUTPUT_SOLUTION, OUTPUT_PRIMITIVE_VARIABLES, OUTPUT_SOURCES)
ALL_VARS = OUTPUT_SOLUTION | OUTPUT_PRIMITIVE_VARIABLES | OUTPUT_SOURCES
NAN = np.array([0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)[0]
SUM_KEYS = ("l1", "l2_squared", "linf")


def _setup(name, B, src=SRC):
    """(operator with B members set, their cases, the state [B, num_cells, 3] as a numpy array of its own)"""
    members = _members(name, src, B)
    op = _operator(name, src, members)
    return op, [c for c, _, _, _ in members], np.stack([c.u_local for c, _, _, _ in members])


def _plant_patterns(u):
    """-0.0, a NaN with a payload and a denormal in every component of some member"""
    B, n, _ = u.shape
    for i, v in enumerate((-0.0, NAN, 5e-324, -1e-310)):
        for c in range(3):
            u[(i + c) % B, (7 * i + 3 * c + 1) % n, c] = v
    return u


def _same_sums(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in SUM_KEYS) and _bits(a["area"]) == _bits(b["area"])


def _device_bytes(op):
    return op.layout_info()["device_bytes"]


def _err_workgroups(no):
    return min((no + 255) // 256, 1024)


@pytest.mark.parametrize("name,B", CONFIGS)
def test_planes_are_the_planes_of_every_members_slice(name, B):
    """every mask 1..7, device form and host form, a state with -0.0, a NaN payload and denormals in it; the device bytes grow by
    8 B k o for the widest mask begun so far and by nothing for the device form"""
    torch = _torch()
    op, cases, un = _setup(name, B)
    no = cases[0].mesh.num_owned_cells
    u = _dev(_plant_patterns(un))
    base = _device_bytes(op)
    widest = 0
    for comps in (1, 2, 4, 3, 5, 6, 7):
        k = bin(comps).count("1")
        got = op.ensemble_state_planes(u, comps)
        assert _device_bytes(op) == base + 8 * B * widest * no
        want = torch.stack([op.state_planes(u[m], comps) for m in range(B)])
        assert got.shape == (B, k, no) and np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))
        op.ensemble_read_state_begin(u, comps)
        widest = max(widest, k)
        bits = [1 << c for c in range(3) if comps >> c & 1]
        for m in range(B):
            for j, comp in enumerate(bits):
                assert np.array_equal(_bits(op.ensemble_read_state(m, comp)), _bits(want[m, j].cpu().numpy())), (comps, m, comp)
        assert op.ensemble_read_state_ready()
        assert _device_bytes(op) == base + 8 * B * widest * no
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    assert np.array_equal(_bits(op.ensemble_state_planes(u, 7).cpu().numpy()), _bits(np.transpose(un[:, own, :], (0, 2, 1))))
    op.destroy()


def test_a_read_is_ordered_in_its_stream_and_replaced_by_a_later_begin():
    """begin, then a launch that overwrites u: the values at begin arrive.  A begin over a read that has not landed: the later one
    arrives.  The pointer form shows the same pinned memory."""
    torch = _torch()
    op, cases, un = _setup("part-o2l", 3)
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    no = own.size
    u = _dev(un)
    op.ensemble_read_state_begin(u, COMPONENT_H | COMPONENT_HV)
    u.fill_(-7.0)
    for m in range(3):
        assert np.array_equal(_bits(op.ensemble_read_state(m, COMPONENT_HV)), _bits(un[m, own, 2]))
        assert np.array_equal(_bits(op.ensemble_read_state(m, COMPONENT_H)), _bits(un[m, own, 0]))
    u2n = un[::-1] * 1.5 + 0.25
    u2 = _dev(u2n)
    op.ensemble_read_state_begin(u, COMPONENT_HU)          # never waited for
    op.ensemble_read_state_begin(u2, COMPONENT_HU | COMPONENT_HV)
    for m in range(3):
        assert np.array_equal(_bits(op.ensemble_read_state(m, COMPONENT_HU)), _bits(u2n[m, own, 1]))
    p = _lib.c_double_p()
    _lib.check(_lib.load().rdyhip_ens_state_read_ptr(op._h, 2, COMPONENT_HV, C.byref(p)))
    assert np.array_equal(_bits(np.ctypeslib.as_array(p, (no,))), _bits(u2n[2, own, 2]))
    with pytest.raises(RDyHipError) as e:
        op.ensemble_read_state(0, COMPONENT_H)            # not among the planes of the last begin
    assert e.value.code == 83
    op.destroy()


def test_the_swe_read_out_of_the_same_operator_is_undisturbed():
    """an SWE read begun before an ensemble read and waited for after it delivers its own values, and the other way round"""
    _torch()
    op, cases, un = _setup("part-o2l", 3)
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    u = _dev(un)
    alone = _dev(un[1] * 2.0 - 0.5)
    op.read_state_begin(alone, 7)
    op.ensemble_read_state_begin(u, 7)
    for m in range(3):
        for c in range(3):
            assert np.array_equal(_bits(op.ensemble_read_state(m, 1 << c)), _bits(un[m, own, c]))
    for c in range(3):
        assert np.array_equal(_bits(op.read_state(1 << c)), _bits((un[1] * 2.0 - 0.5)[own, c]))
    op.ensemble_read_state_begin(u, COMPONENT_HU)
    op.read_state_begin(u[2], COMPONENT_H)
    assert np.array_equal(_bits(op.read_state(COMPONENT_H)), _bits(un[2, own, 0]))
    assert np.array_equal(_bits(op.ensemble_read_state(0, COMPONENT_HU)), _bits(un[0, own, 1]))
    op.destroy()


@pytest.mark.parametrize("name,B", CONFIGS)
def test_error_sums_are_the_sums_of_every_members_slice(name, B):
    """with and without an exact state; the SWE result of the same operator is left as it was; the device bytes grow by
    80 B (G + 1), the area table and the SWE records having been allocated by the SWE call before"""
    _torch()
    op, cases, un = _setup(name, B)
    no = cases[0].mesh.num_owned_cells
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    u = _dev(un)
    exn = un[:, own, :] * 0.75 + 0.01 * np.arange(B)[:, None, None]
    ex = _dev(exn)
    want = [op.error_sums(u[m]) for m in range(B)]
    want_ex = [op.error_sums(u[m], ex[m]) for m in range(B)]
    swe = _lib.RDyHipErrorSums()
    _lib.check(_lib.load().rdyhip_error_sums_get(op._h, C.byref(swe)))
    base = _device_bytes(op)
    got = op.ensemble_error_sums(u)
    assert _device_bytes(op) == base + 80 * B * (_err_workgroups(no) + 1)
    got_ex = op.ensemble_error_sums(u, ex)
    assert _device_bytes(op) == base + 80 * B * (_err_workgroups(no) + 1)
    assert len(got) == len(got_ex) == B
    for m in range(B):
        assert _same_sums(got[m], want[m]) and _same_sums(got_ex[m], want_ex[m]), m
        assert got[m]["l1"][0] > 0.0 and got[m]["area"] > 0.0
    after = _lib.RDyHipErrorSums()
    _lib.check(_lib.load().rdyhip_error_sums_get(op._h, C.byref(after)))
    assert bytes(swe) == bytes(after) and np.array_equal(_bits(np.array(after.l1[:])), _bits(want_ex[B - 1]["l1"]))
    op.destroy()


@functools.lru_cache(maxsize=None)
def _mesh_beyond_one_finalize_round():
    mesh = M.structured_tri_mesh(182, 182, 1.0, zfunc=_bathymetry)
    assert mesh.num_owned_cells == 66248 > 65536
    return mesh


def test_error_sums_beyond_one_finalize_round():
    """66 248 owned cells: 259 workgroups per member, so lanes 0..2 of the finalize fold take a second record"""
    _torch()
    mesh = _mesh_beyond_one_finalize_round()
    no, B = mesh.num_owned_cells, 2
    assert _err_workgroups(no) == 259
    rng = np.random.default_rng(66248)
    un = rng.uniform(-1.0, 1.0, (B, mesh.num_cells, 3))
    un[:, :, 0] = np.abs(un[:, :, 0])
    exn = rng.uniform(-1.0, 1.0, (B, no, 3))
    op = Operator.create(RDyFlowConfig(), mesh)
    op.enable_ensemble(B)
    u, ex = _dev(un), _dev(exn)
    got, got_ex = op.ensemble_error_sums(u), op.ensemble_error_sums(u, ex)
    for m in range(B):
        assert _same_sums(got[m], op.error_sums(u[m])) and _same_sums(got_ex[m], op.error_sums(u[m], ex[m])), m
    assert not _same_sums(got[0], got[1])
    op.destroy()


def _lifted(un):
    """the members' states under one more metre of water: no dry cell, so forward Euler steps from them stay finite (the members'
    own states have dry cells beside wet ones, from which a plain Euler step takes depths below zero and the next one makes NaN)"""
    out = un.copy()
    out[:, :, 0] += 1.0
    return out


def _run_means(op, cases, un, dts_of_step, set_source=True):
    """the ensemble path and the per-operator path over the states s_0 = the members' own (dry cells, films, deep water), s_1 = the
    same under one more metre of water, s_(k+1) = one Euler step of all members from s_k with dts_of_step[k]; accumulate k takes
    s_(k+1) as the solution and s_k as the state of the primitive variables, weighted with dts_of_step[k].  Returns ((means, times)
    per variable of the ensemble path, the same of the per-operator path).  The per-operator path, one member at a time on the
    same operator: the operator's source set to the member's, then per accumulate an SWE evaluation on the member's slice of s_k
    and accumulate_output_means with the member's slice of s_(k+1); then output_mean and a reset."""
    torch = _torch()
    B = len(cases)
    mesh = cases[0].mesh
    no = mesh.num_owned_cells
    states = [_dev(un), _dev(_lifted(un))]
    op.ensemble_enable_output_means(ALL_VARS)
    op.ensemble_accumulate_output_means(ALL_VARS, dts_of_step[0], states[1], states[0])
    for d in dts_of_step[1:]:
        nxt = states[-1].clone()
        op.ensemble_euler_step(d, states[-1], nxt)
        op.ensemble_accumulate_output_means(ALL_VARS, d, nxt, states[-1])
        states.append(nxt)
    torch.cuda.synchronize()
    assert all(np.isfinite(s.cpu().numpy()).all() for s in states)
    assert not np.array_equal(states[-1].cpu().numpy(), states[1].cpu().numpy())
    ens = {var: op.ensemble_output_mean(var) for var in VARS}
    op.enable_output_means(ALL_VARS)
    f = torch.empty((no, 3), dtype=torch.float64, device="cuda")
    per = {var: ([], []) for var in VARS}
    for m in range(B):
        if set_source:
            for comp in range(3):
                op.set_domain_external_source(comp, cases[m].ext_src[:, comp])
        for s, d in enumerate(dts_of_step):
            op.rhs_function(float(d[m]), states[s][m], f)
            op.accumulate_output_means(ALL_VARS, float(d[m]), states[s + 1][m])
        for var in VARS:
            mean, t = op.output_mean(var)
            per[var][0].append(mean.cpu().numpy())
            per[var][1].append(t)
        op.reset_output_means(ALL_VARS)
    return ens, per


def _check_means(ens, per, B):
    for var in VARS:
        mean, times = ens[var]
        assert np.array_equal(_bits(times), _bits(np.array(per[var][1]))), var
        got = mean.cpu().numpy()
        for m in range(B):
            assert np.array_equal(_bits(got[m]), _bits(per[var][0][m])), (var, m)
        assert np.abs(got).max() > 0.0


def _dts(cases, steps):
    """one accumulate of the members' own states, then `steps` Euler steps with dts distinct per member, one member's 0.0
    (B >= 3), and a last step in which every member has a dt: a member without accumulated time has no mean on either path
    (test_means_of_solution... and test_means_refusals_and_reset check that), so the member that stood still moves once before the
    means are compared"""
    B = len(cases)
    d = np.array([1e-3 * (1.0 + 0.25 * m) for m in range(B)])
    first, last = d * 0.75, d * 0.5
    if B >= 3:
        d[B // 2] = 0.0
        first[B // 2] = 0.0
    return [first] + [d.copy() for _ in range(steps)] + [last]


@pytest.mark.parametrize("name,B", CONFIGS)
def test_means_of_solution_primitive_variables_and_sources(name, B):
    """an accumulate of the members' own states and 5 Euler steps with distinct dts per member, one member's 0.0 (its accumulators
    go through six fma(0, x, acc) and its time stays 0: its mean is then refused), then one step in which every member moves: all
    three means and times of every member are the bits of the per-operator path with the operator's source set to the member's"""
    op, cases, un = _setup(name, B)
    no = cases[0].mesh.num_owned_cells
    base = _device_bytes(op)
    dts = _dts(cases, 5)
    if B >= 3:
        # the state after the five steps: member B // 2 has accumulated nothing and is refused, by both paths, and nothing is written
        op.ensemble_enable_output_means(ALL_VARS)
        u = _dev(un)
        op.ensemble_accumulate_output_means(ALL_VARS, dts[0], u, u)
        assert op.ensemble_output_mean_time(OUTPUT_SOLUTION)[B // 2] == 0.0
        with pytest.raises(RDyHipError) as e:
            op.ensemble_output_mean(OUTPUT_SOLUTION)
        assert e.value.code == 83 and f"member {B // 2}" in e.value.message
        op.ensemble_reset_output_means(ALL_VARS)
        assert (op.ensemble_output_mean_time(OUTPUT_SOLUTION) == 0.0).all()
    ens, per = _run_means(op, cases, un, dts)
    assert _device_bytes(op) == base + 3 * 24 * B * no + 3 * 24 * no            # the three ensemble accumulators and the three SWE ones
    _check_means(ens, per, B)
    want_t = np.zeros(B)
    for d in dts:
        want_t = want_t + d
    assert np.array_equal(_bits(ens[OUTPUT_SOLUTION][1]), _bits(want_t))
    op.destroy()


def test_means_where_solution_and_primitive_state_are_one_array():
    """u_solution == u_primitive: the row is read once; the bits are those of two different arrays with the same content"""
    _torch()
    op, cases, un = _setup("part-o2l", 3)
    d = np.array([0.1, 0.2, 0.3])
    u, v = _dev(un), _dev(un)
    op.ensemble_enable_output_means(3)
    op.ensemble_accumulate_output_means(3, d, u, u)
    a = {var: op.ensemble_output_mean(var)[0].cpu().numpy() for var in VARS[:2]}
    op.ensemble_reset_output_means(3)
    op.ensemble_accumulate_output_means(3, d, u, v)
    for var in VARS[:2]:
        assert np.array_equal(_bits(a[var]), _bits(op.ensemble_output_mean(var)[0].cpu().numpy()))
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    # (values, not bits: fma(d, -0.0, +0.0) is +0.0 where the product d * -0.0 is -0.0)
    assert np.array_equal(a[OUTPUT_SOLUTION], (d[:, None, None] * un[:, own, :]) * (1.0 / d)[:, None, None])
    op.destroy()


def test_means_refusals_and_reset():
    """a mean asked for before any accumulate is refused and nothing changes; a reset of one variable leaves the others"""
    torch = _torch()
    op, cases, un = _setup("mixed", 3)
    no = cases[0].mesh.num_owned_cells
    u = _dev(un)
    op.ensemble_enable_output_means(OUTPUT_SOLUTION | OUTPUT_SOURCES)
    lib = _lib.load()
    out = torch.full((3, no, 3), 5.0, dtype=torch.float64, device="cuda")
    t = np.full(3, -1.0)
    tp = t.ctypes.data_as(_lib.c_double_p)
    assert lib.rdyhip_ens_output_mean_get(op._h, OUTPUT_SOLUTION, out.data_ptr(), tp, None) == 83
    assert b"no accumulated time" in lib.rdyhip_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all() and (t == -1.0).all()
    # a variable that is not enabled, unknown bits, two variables where one is asked for
    for call in (lambda: op.ensemble_accumulate_output_means(OUTPUT_PRIMITIVE_VARIABLES, [0.1] * 3, u, u), lambda: op.ensemble_output_mean(OUTPUT_PRIMITIVE_VARIABLES),
                 lambda: op.ensemble_reset_output_means(ALL_VARS), lambda: op.ensemble_output_mean_time(OUTPUT_PRIMITIVE_VARIABLES),
                 lambda: op.ensemble_enable_output_means(8), lambda: op.ensemble_output_mean(OUTPUT_SOLUTION | OUTPUT_SOURCES),
                 lambda: op.ensemble_output_mean(0)):
        with pytest.raises(RDyHipError) as e:
            call()
        assert e.value.code == 83
    d = np.array([0.25, 0.5, 1.0])
    op.ensemble_accumulate_output_means(OUTPUT_SOLUTION | OUTPUT_SOURCES, d, u)
    op.ensemble_accumulate_output_means(OUTPUT_SOURCES, d)
    assert np.array_equal(op.ensemble_output_mean_time(OUTPUT_SOLUTION), d) and np.array_equal(op.ensemble_output_mean_time(OUTPUT_SOURCES), 2 * d)
    src, ts = op.ensemble_output_mean(OUTPUT_SOURCES)
    assert np.array_equal(ts, 2 * d)
    want = np.stack([c.ext_src for c in cases])
    acc = d[:, None, None] * want
    acc = d[:, None, None] * want + acc                    # fma(d, x, fma(d, x, 0)) of binary fractions d: exact products
    assert np.array_equal(src.cpu().numpy(), acc * (1.0 / (2 * d))[:, None, None])
    op.ensemble_reset_output_means(OUTPUT_SOLUTION)
    assert (op.ensemble_output_mean_time(OUTPUT_SOLUTION) == 0.0).all() and np.array_equal(op.ensemble_output_mean_time(OUTPUT_SOURCES), 2 * d)
    with pytest.raises(RDyHipError):
        op.ensemble_output_mean(OUTPUT_SOLUTION)
    assert np.array_equal(_bits(op.ensemble_output_mean(OUTPUT_SOURCES)[0].cpu().numpy()), _bits(src.cpu().numpy()))
    op.ensemble_accumulate_output_means(OUTPUT_SOLUTION, d, u)
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    assert np.array_equal(op.ensemble_output_mean(OUTPUT_SOLUTION)[0].cpu().numpy(), (d[:, None, None] * un[:, own, :]) * (1.0 / d)[:, None, None])
    # a second enable keeps the content
    op.ensemble_enable_output_means(ALL_VARS)
    assert np.array_equal(op.ensemble_output_mean_time(OUTPUT_SOURCES), 2 * d) and (op.ensemble_output_mean_time(OUTPUT_PRIMITIVE_VARIABLES) == 0.0).all()
    op.destroy()


def test_means_under_hydrostatic_reconstruction(rdyhip_kernel, monkeypatch):
    """after enable_ensemble(B, well_balancing=2) on part-o2l with bed elevations: the family makes no difference to the output.
    (An operator with hydrostatic reconstruction cannot be created under RDYHIP_KERNEL=cell, which the suite's autouse fixture
    sets for every second run: the variable is taken out, as test_gpu_ensemble_hr.py does.)"""
    monkeypatch.delenv("RDYHIP_KERNEL", raising=False)
    name, src, B = "part-o2l", SOURCE_IMPLICIT_XQ2018, 3
    members = hr_members(name, src, B)
    cases = [c for c, _, _, _ in members]
    op = Operator.create(cases[0].config, cases[0].mesh, cases[0].condition_types)
    op.enable_ensemble(B, well_balancing=WELL_BALANCING_HR)
    assert op.ensemble_well_balancing() == WELL_BALANCING_HR
    for m, c in enumerate(cases):
        _set_member(op, m, c)
    un = np.stack([c.u_local for c in cases])
    ens, per = _run_means(op, cases, un, _dts(cases, 5))
    _check_means(ens, per, B)
    u = _dev(un)
    got = op.ensemble_stats(u, 7).cpu().numpy()
    own = np.asarray(cases[0].mesh.cell_owned_to_local)
    for c in range(3):
        assert np.array_equal(_bits(got[c]), _bits(ensemble_stats_rule(un[:, own, c])))
    op.destroy()


@pytest.mark.parametrize("name,B", [("part-o2l", 3), ("quad-44", 7), ("tri-30", 1)])
def test_series_records_are_the_rows_of_the_members_states(name, B):
    torch = _torch()
    op, cases, un = _setup(name, B)
    mesh = cases[0].mesh
    no = mesh.num_owned_cells
    own = np.asarray(mesh.cell_owned_to_local)
    sites = np.array([no - 1, 0, 5, no - 1, 17 % no, 5], dtype=np.int32)       # repeats
    S, cap = sites.size, 3
    base = _device_bytes(op)
    op.ensemble_enable_observation_series(sites, cap)
    assert _device_bytes(op) == base + 24 * B * S * cap + 4 * S
    assert op.ensemble_series_info() == {"entries": S, "count": 0, "capacity": cap}
    states, times = [], []
    for r in range(cap):
        s = un * (1.0 + 0.5 * r) - 0.125 * r
        u = _dev(s)
        t = np.array([10.0 * r + m for m in range(B)])
        op.ensemble_series_record(t, u)
        u.fill_(99.0)                                      # the record was taken at its place in the stream
        states.append(s)
        times.append(t)
    # a full log: refused, nothing launched, nothing counted
    with pytest.raises(RDyHipError) as e:
        op.ensemble_series_record(np.zeros(B), _dev(un))
    assert e.value.code == 83 and "full" in e.value.message and op.ensemble_series_info()["count"] == cap
    tt, vv = op.ensemble_series_read()
    assert tt.shape == (cap, B) and vv.shape == (cap, B, S, 3)
    assert np.array_equal(tt, np.stack(times))
    for r in range(cap):
        assert np.array_equal(_bits(vv[r]), _bits(states[r][:, own[sites], :])), r
    t1, v1 = op.ensemble_series_read(1, 2)
    assert np.array_equal(t1, tt[1:]) and np.array_equal(_bits(v1), _bits(vv[1:]))
    lib = _lib.load()
    for first, count in ((-1, 1), (0, cap + 1), (2, 2), (0, -1)):
        assert lib.rdyhip_ens_series_read(op._h, first, count, tt.ctypes.data_as(_lib.c_double_p), vv.ctypes.data_as(_lib.c_double_p), None) == 83
    op.ensemble_series_clear()
    assert op.ensemble_series_info()["count"] == 0
    op.ensemble_series_record(times[2], _dev(states[1]))
    t2, v2 = op.ensemble_series_read()
    assert np.array_equal(t2, times[2][None]) and np.array_equal(_bits(v2[0]), _bits(states[1][:, own[sites], :]))
    with pytest.raises(RDyHipError) as e:
        op.ensemble_enable_observation_series(sites, cap)
    assert e.value.code == 83 and "already" in e.value.message
    torch.cuda.synchronize()
    op.destroy()


def test_a_series_without_sites():
    _torch()
    op, cases, un = _setup("tri-30", 3)
    base = _device_bytes(op)
    op.ensemble_enable_observation_series([], 2)
    assert _device_bytes(op) == base
    op.ensemble_series_record([1.0, 2.0, 3.0], _dev(un))
    assert _lib.load().rdyhip_ens_series_record(op._h, np.arange(3.0).ctypes.data_as(_lib.c_double_p), None, None) == 0
    t, v = op.ensemble_series_read()
    assert np.array_equal(t, [[1.0, 2.0, 3.0], [0.0, 1.0, 2.0]]) and v.shape == (2, 3, 0, 3)
    with pytest.raises(RDyHipError):
        op.ensemble_series_record([0.0] * 3, _dev(un))
    op.destroy()


@pytest.mark.parametrize("name,B", CONFIGS)
def test_statistics_are_the_rule_of_the_cpu_file(name, B):
    """every mask; from three members on the hand-made columns of the CPU test (signed zeros, a tie, a NaN in member 0 and in a later
    member, denormals) are planted -- on part-o2l at owned cells whose local id differs from the owned id"""
    _torch()
    op, cases, un = _setup(name, B)
    mesh = cases[0].mesh
    no = mesh.num_owned_cells
    own = np.asarray(mesh.cell_owned_to_local)
    if B >= 3:
        x = planted_rows(B)
        cand = np.nonzero(own != np.arange(no))[0] if name == "part-o2l" else np.arange(no)
        assert cand.size >= x.shape[1]
        at = cand[np.linspace(0, cand.size - 1, x.shape[1]).astype(int)]
        assert np.unique(at).size == x.shape[1]
        for c in range(3):
            un[:, own[np.roll(at, c)], c] = x
    u = _dev(un)
    want = np.stack([ensemble_stats_rule(un[:, own, c]) for c in range(3)])
    if B >= 3:
        assert np.isnan(want[:, 0]).any() and (_bits(want[:, 1]) == _bits(-0.0)).any()
    base = _device_bytes(op)
    for comps in range(1, 8):
        got = op.ensemble_stats(u, comps).cpu().numpy()
        sel = [c for c in range(3) if comps >> c & 1]
        assert got.shape == (len(sel), 3, no) and np.array_equal(_bits(got), _bits(want[sel])), comps
    assert _device_bytes(op) == base
    op.destroy()


def test_the_stepper_with_means_and_series_and_with_its_defaults():
    """EnsembleEulerStepper(op, means=7, series=...) over 10 steps: states, means and records are those of explicit calls; with the
    defaults the states are the bits of a plain loop of ensemble_euler_step and no output call is made"""
    torch = _torch()
    name, B, steps = "part-o2l", 3, 10
    op, cases, un = _setup(name, B)
    ex, _, _ = _setup(name, B)
    un = _lifted(un)
    no = cases[0].mesh.num_owned_cells
    d = np.array([1e-3 * (1.0 + 0.25 * m) for m in range(B)])
    sites = [3, no - 1, 3]
    # explicit calls
    ex.ensemble_enable_output_means(ALL_VARS)
    ex.ensemble_enable_observation_series(sites, 8)
    a, b = _dev(un), _dev(un)
    t = np.zeros(B)
    for s in range(1, steps + 1):
        ex.ensemble_euler_step(d, a, b)
        ex.ensemble_accumulate_output_means(ALL_VARS, d, b, a)
        a, b = b, a
        t = t + d
        if s % 3 == 0:
            ex.ensemble_series_record(t, a)
    torch.cuda.synchronize()
    want_state = a.cpu().numpy()
    assert np.isfinite(want_state).all()
    # the stepper
    st = EnsembleEulerStepper(op, means=ALL_VARS, series=TimeSeries(observation_sites=sites, observation_interval=3, capacity=8))
    u = st.advance(_dev(un), d, 4)
    u = st.advance(u, d, steps - 4)
    torch.cuda.synchronize()
    assert st.step == steps and np.array_equal(_bits(st.times), _bits(t))
    assert np.array_equal(_bits(u.cpu().numpy()), _bits(want_state))
    tt, vv = st.series_read(clear=True)
    et, ev = ex.ensemble_series_read()
    assert tt.shape == (3, B) and np.array_equal(_bits(tt), _bits(et)) and np.array_equal(_bits(vv), _bits(ev))
    assert op.ensemble_series_info()["count"] == 0
    for var in VARS:
        mean, times = st.output_mean(var)
        emean, etimes = ex.ensemble_output_mean(var)
        assert np.array_equal(_bits(times), _bits(etimes)) and np.array_equal(_bits(mean.cpu().numpy()), _bits(emean.cpu().numpy())), var
        assert (op.ensemble_output_mean_time(var) == 0.0).all()       # the next window starts empty
    op.destroy()
    ex.destroy()
    # the defaults: today's stepper
    op, _, _ = _setup(name, B)
    base = _device_bytes(op)
    st = EnsembleEulerStepper(op)
    assert st.means == 0 and st.series is None
    u = st.advance(_dev(un), d, steps)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(u.cpu().numpy()), _bits(want_state)) and _device_bytes(op) == base
    with pytest.raises(RDyHipError):
        op.ensemble_series_info()
    with pytest.raises(RDyHipError):
        op.ensemble_output_mean_time(OUTPUT_SOLUTION)
    op.destroy()


def test_refusals():
    torch = _torch()
    lib = _lib.load()
    case = _members("tri-30", SRC, 1)[0][0]
    mesh = case.mesh
    no = mesh.num_owned_cells
    vals = np.zeros(64 * 3 * max(no, 8))
    vp = vals.ctypes.data_as(_lib.c_double_p)
    ids = np.zeros(4, dtype=np.int32)
    ip = ids.ctypes.data_as(_lib.c_int32_p)
    i = C.c_int32()
    p = _lib.c_double_p()
    sums = (_lib.RDyHipErrorSums * 64)()
    u = torch.zeros((2, mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    out = torch.zeros((2, 3, 3, no), dtype=torch.float64, device="cuda")
    up, op_ = u.data_ptr(), out.data_ptr()
    # each call before an enable
    op = Operator.create(case.config, mesh, case.condition_types)
    before = {
        "state_planes": (7, up, op_, None), "state_read_begin": (7, up, None), "state_read_ready": (C.byref(i),), "state_read_wait": (),
        "state_read_get": (0, 1, no, vp), "state_read_ptr": (0, 1, C.byref(p)), "error_sums": (up, None, None), "error_sums_get": (sums,),
        "output_mean_enable": (7,), "output_mean_accumulate": (7, vp, up, up, None), "output_mean_get": (1, op_, vp, None),
        "output_mean_reset": (7, None), "output_mean_time": (1, vp), "series_enable": (2, ip, 4), "series_record": (vp, up, None),
        "series_info": (C.byref(i), C.byref(i), C.byref(i)), "series_read": (0, 0, vp, vp, None), "series_clear": (), "stats": (7, up, op_, None)}
    for name, args in before.items():
        assert getattr(lib, "rdyhip_ens_" + name)(op._h, *args) == 83, name
        assert b"not enabled" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())
    base = _device_bytes(op)
    op.enable_ensemble(2)
    base2 = _device_bytes(op)
    # a mask out of range, a null array where one is needed
    for comps in (0, 8, -1):
        assert lib.rdyhip_ens_state_planes(op._h, comps, up, op_, None) == 83
        assert lib.rdyhip_ens_state_read_begin(op._h, comps, up, None) == 83
        assert lib.rdyhip_ens_stats(op._h, comps, up, op_, None) == 83
    for a, b in ((None, op_), (up, None)):
        assert lib.rdyhip_ens_state_planes(op._h, 7, a, b, None) == 83 and lib.rdyhip_ens_stats(op._h, 7, a, b, None) == 83
    assert lib.rdyhip_ens_state_read_begin(op._h, 7, None, None) == 83
    assert lib.rdyhip_ens_error_sums(op._h, None, None, None) == 83 and lib.rdyhip_ens_error_sums_get(op._h, None) == 83
    # the read-out's state machine: nothing begun; begun but not waited for; a member or component out of range; a wrong size
    assert lib.rdyhip_ens_state_read_ready(op._h, C.byref(i)) == 83 and lib.rdyhip_ens_state_read_wait(op._h) == 83
    assert lib.rdyhip_ens_state_read_get(op._h, 0, 1, no, vp) == 83 and lib.rdyhip_ens_state_read_ptr(op._h, 0, 1, C.byref(p)) == 83
    assert lib.rdyhip_ens_error_sums_get(op._h, sums) == 83 and b"no ensemble error sums" in lib.rdyhip_last_error()
    assert lib.rdyhip_ens_state_read_ready(op._h, None) == 83
    op.ensemble_read_state_begin(u, COMPONENT_H | COMPONENT_HU)
    assert lib.rdyhip_ens_state_read_get(op._h, 0, 1, no, vp) == 83 and b"not been waited for" in lib.rdyhip_last_error()
    assert lib.rdyhip_ens_state_read_wait(op._h) == 0
    for member in (-1, 2):
        assert lib.rdyhip_ens_state_read_get(op._h, member, 1, no, vp) == 83 and b"member index" in lib.rdyhip_last_error()
        assert lib.rdyhip_ens_state_read_ptr(op._h, member, 1, C.byref(p)) == 83
    for comp in (0, 3, 8):
        assert lib.rdyhip_ens_state_read_get(op._h, 0, comp, no, vp) == 83 and lib.rdyhip_ens_state_read_ptr(op._h, 0, comp, C.byref(p)) == 83
    assert lib.rdyhip_ens_state_read_get(op._h, 0, COMPONENT_HV, no, vp) == 83 and b"was not asked for" in lib.rdyhip_last_error()
    for size in (no - 1, no + 1, 0):
        assert lib.rdyhip_ens_state_read_get(op._h, 0, 1, size, vp) == 60
    assert lib.rdyhip_ens_state_read_get(op._h, 0, 1, no, None) == 83 and lib.rdyhip_ens_state_read_ptr(op._h, 0, 1, None) == 83
    assert lib.rdyhip_ens_state_read_get(op._h, 1, 2, no, vp) == 0
    # the means: null arrays
    op.ensemble_enable_output_means(ALL_VARS)
    assert lib.rdyhip_ens_output_mean_accumulate(op._h, 7, None, up, up, None) == 83
    assert lib.rdyhip_ens_output_mean_accumulate(op._h, 1, vp, None, up, None) == 83
    assert lib.rdyhip_ens_output_mean_accumulate(op._h, 2, vp, up, None, None) == 83
    assert lib.rdyhip_ens_output_mean_time(op._h, 1, None) == 83
    assert lib.rdyhip_ens_output_mean_accumulate(op._h, 4, np.ones(2).ctypes.data_as(_lib.c_double_p), None, None, None) == 0
    assert lib.rdyhip_ens_output_mean_get(op._h, 4, None, vp, None) == 83
    assert lib.rdyhip_ens_output_mean_get(op._h, 4, op_, None, None) == 0            # the times may be NULL
    # the series: a site out of range, negative counts, a null list, null times
    for bad in (-1, no):
        ids[:] = (0, bad, 1, 2)
        assert lib.rdyhip_ens_series_enable(op._h, 4, ip, 2) == 83 and b"out of range" in lib.rdyhip_last_error()
    ids[:] = 0
    assert lib.rdyhip_ens_series_enable(op._h, -1, ip, 2) == 83 and lib.rdyhip_ens_series_enable(op._h, 1, ip, -2) == 83
    assert lib.rdyhip_ens_series_enable(op._h, 1, None, 2) == 83
    assert lib.rdyhip_ens_series_enable(op._h, 2, ip, 2) == 0
    assert lib.rdyhip_ens_series_record(op._h, None, up, None) == 83 and lib.rdyhip_ens_series_record(op._h, vp, None, None) == 83
    assert lib.rdyhip_ens_series_record(op._h, vp, up, None) == 0
    assert lib.rdyhip_ens_series_read(op._h, 0, 1, None, vp, None) == 83 and lib.rdyhip_ens_series_read(op._h, 0, 1, vp, None, None) == 83
    assert lib.rdyhip_ens_series_read(op._h, 0, 1, vp, vp, None) == 0
    # the Python mirror's shape checks
    for call in (lambda: op.ensemble_state_planes(u[:1], 7), lambda: op.ensemble_stats(u.float(), 7), lambda: op.ensemble_read_state_begin(u.cpu(), 7),
                 lambda: op.ensemble_error_sums(u, u[:1]), lambda: op.ensemble_accumulate_output_means(1, [0.1], u, u),
                 lambda: op.ensemble_series_record([0.1, 0.2, 0.3], u)):
        with pytest.raises(RDyHipError) as e:
            call()
        assert e.value.code == 83
    torch.cuda.synchronize()
    # what the calls above allocated, by the formulas of the header: the read-out's planes (2 components), the three accumulators,
    # the log and the sites; no error sums were launched
    assert _device_bytes(op) == base2 + 8 * 2 * 2 * no + 3 * 24 * 2 * no + (24 * 2 * 2 * 2 + 4 * 2) and base2 > base
    op.destroy()


def test_a_rank_that_owns_nothing():
    torch = _torch()
    mesh = _empty_mesh()
    B = 3
    op = Operator.create(RDyFlowConfig(), mesh)
    op.enable_ensemble(B)
    base = _device_bytes(op)
    u = torch.zeros((B, mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    assert op.ensemble_state_planes(u, 7).shape == (B, 3, 0) and op.ensemble_stats(u, 5).shape == (2, 3, 0)
    op.ensemble_read_state_begin(u, 7)
    assert op.ensemble_read_state_ready() and op.ensemble_read_state(2, COMPONENT_HV).shape == (0,)
    assert _lib.load().rdyhip_ens_state_read_get(op._h, 0, 1, 1, None) == 60
    sums = op.ensemble_error_sums(u)
    assert len(sums) == B and all(s["area"] == 0.0 and not s["l1"].any() and not s["linf"].any() for s in sums)
    op.ensemble_enable_output_means(ALL_VARS)
    d = np.array([0.5, 0.25, 1.0])
    op.ensemble_accumulate_output_means(ALL_VARS, d, u, u)
    op.ensemble_accumulate_output_means(OUTPUT_SOURCES, d)
    mean, t = op.ensemble_output_mean(OUTPUT_SOURCES)
    assert mean.shape == (B, 0, 3) and np.array_equal(t, 2 * d) and np.array_equal(op.ensemble_output_mean_time(OUTPUT_SOLUTION), d)
    op.ensemble_reset_output_means(OUTPUT_SOURCES)
    assert (op.ensemble_output_mean_time(OUTPUT_SOURCES) == 0.0).all()
    with pytest.raises(RDyHipError):
        op.ensemble_enable_observation_series([0], 2)      # no owned cell to observe
    op.ensemble_enable_observation_series([], 2)
    op.ensemble_series_record(d, u)
    tt, vv = op.ensemble_series_read()
    assert np.array_equal(tt, d[None]) and vv.shape == (1, B, 0, 3)
    st = EnsembleEulerStepper(op, means=OUTPUT_SOLUTION)
    st.advance(u, d, 2)
    assert np.array_equal(op.ensemble_output_mean_time(OUTPUT_SOLUTION), d + d + d)
    torch.cuda.synchronize()
    assert _device_bytes(op) == base
    op.destroy()
