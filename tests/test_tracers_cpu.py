"""CPU: shallow water with advected tracers (rdyhip_tracers_*, csrc/tracer_kernels.h) as far as it goes without a device --
the numpy reference the GPU tests compare against (tests/tracer_reference.py) is tied to the C oracle, to a hand-derived
answer and to the reference's sediment convergence study; the new entry points report a null operator before any device
call; and every instantiation of the kernel in the built library keeps its rows in registers."""
import ctypes as C

import numpy as np
import pytest

import mms
import random_cases as RC
import tracer_reference as TR
from helpers import oracle_from_case, rel_linf
from rdycore_amd import _lib, build, codeobj
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig


def tracer_case(rng, mesh, nt, riemann, tiny=True, h_anuga=0.0, region_block=0, tiny_h=None):
    """a random_case of the SWE fuzz tests (wet / dry / thin films, friction, slopes, sources, Dirichlet data; region_block > 0:
    the classes of cell in runs, which makes wet/dry fronts) with its critical-outflow boundaries made reflecting, widened by
    `nt` tracers; returns (case, reference, state [num_cells, 3 + nt]).  tiny_h: the wet/dry threshold, None: the default of
    RDyFlowConfig.  Also used by the GPU tests of the tracer kernel."""
    cfg = RDyFlowConfig(h_anuga_regular=h_anuga) if tiny_h is None else RDyFlowConfig(h_anuga_regular=h_anuga, tiny_h=tiny_h)
    case = RC.random_case(rng, mesh, cfg, region_block=region_block)
    case.condition_types = [M.CONDITION_REFLECTING if t == M.CONDITION_CRITICAL_OUTFLOW else t for t in case.condition_types]
    if not tiny:
        case.u_local[case.cell_kind == RC.KIND_TINY] = 0.0
    ref = TR.TracerReference(mesh, case.condition_types, nt, riemann, case.config.tiny_h, case.config.h_anuga_regular)
    ref.mannings[:] = case.mannings
    ref.external_sources[:] = case.ext_src
    ref.tracer_sources[:] = rng.normal(size=(mesh.num_owned_cells, nt)) * 1e-3
    for b, vals in case.boundary_values.items():
        ref.boundary_values[b][:, :3] = vals
        ref.boundary_values[b][:, 3:] = vals[:, :1] * rng.uniform(0.0, 0.8, (vals.shape[0], nt))
    u = np.concatenate([case.u_local, case.u_local[:, :1] * rng.uniform(0.0, 0.8, (mesh.num_cells, nt))], axis=1)
    return case, ref, u


@pytest.mark.parametrize("riemann", [TR.RIEMANN_ROE, TR.RIEMANN_UPWIND_ROE])
@pytest.mark.parametrize("kind,nx,ny", [("tri", 9, 7), ("quad", 8, 6), ("mixed", 8, 8)])
def test_flow_components_are_the_oracles_first_order_rhs(kind, nx, ny, riemann):
    """The flow components of the tracer reference are the first-order semi-implicit SWE right-hand side with h_anuga = 0:
    1e-12 relative (the project's first-order Courant bar) against the pinned C oracle, and the same Courant number."""
    rng = np.random.default_rng(2024 + nx)
    mesh = RC.random_mesh(rng, kind, nx, ny)
    for nt in (1, 3):
        case, ref, u = tracer_case(rng, mesh, nt, riemann)
        assert case.config.h_anuga_regular == 0.0 and (u[:, 0] == 0.0).any() and ((u[:, 0] > 0.0) & (u[:, 0] < case.config.tiny_h)).any()
        assert {M.CONDITION_DIRICHLET, M.CONDITION_REFLECTING} == set(case.condition_types)
        orc = oracle_from_case(case)
        F = ref.apply(case.dt, u)
        Fo = orc.apply(case.dt, case.u_local)
        assert np.isfinite(F).all()
        err = rel_linf(F[:, :3], Fo)
        print(f"{kind} nt={nt} riemann={riemann}: flow components vs oracle {err:.3e}")
        assert err <= 1e-12
        assert rel_linf(ref.primitive_variables[:, :3], orc.primitive_variables) <= 1e-12
        cmax = orc.diagnostics()[0]
        assert abs(ref.courant[0] - cmax) <= 1e-12 * max(1.0, cmax)


@pytest.mark.parametrize("riemann,dry", [(TR.RIEMANN_ROE, True), (TR.RIEMANN_UPWIND_ROE, False)])
def test_uniform_concentration_is_carried_by_the_mass_flux(riemann, dry):
    """A hand-derived answer.  Uniform concentration c, Manning's n = 0, no water and no tracer source: for every wet cell
    F[3 + j] = c F[0] - 0.001 - 0.01 c.  With uniform c the Roe wave strength dW_j = (c hr - c hl) - c (hr - hl) vanishes and
    the tracer flux is c times the mass flux (both variants); with Cd = 0 the bed stress is 0, so e = 0.001 (0 - 0.1) / 0.1 and
    d = 0.01 c.  A dry side (h = 0 exactly, concentration 0 by the wet/dry rule) does not break this for the Roe flux:
    cihat = c and dW_j = -c hl + c hl = 0.  The upwind flux takes the concentration of the side the mass flux comes from, which
    next to a dry cell may be that cell's 0 (Roe's mass flux can leave a dry cell), so its state is wet everywhere.  Cells
    between 0 and tiny_h carry water but concentration 0 and are left out of both.
    Rounding only: a cell sums <= 4 edge terms of magnitude <= T = max(len / area) max(h) (sqrt(g max h) + max |u|) c, each
    formed by a few dozen roundings, so 1e-12 max(1, T) leaves two decimal digits above 4 x 32 x 2^-53 T."""
    rng = np.random.default_rng(77)
    mesh = RC.random_mesh(rng, "mixed", 8, 8)
    conc = np.array([0.3, 0.05])
    case, ref, u = tracer_case(rng, mesh, 2, riemann, tiny=False)
    if not dry:
        u[:, :3] = np.where(u[:, :1] < 0.2, np.array([[1.0, 0.3, -0.2]]), u[:, :3])
    else:
        assert (u[:, 0] == 0.0).any()
    ref.mannings[:] = 0.0
    ref.external_sources[:] = 0.0
    ref.tracer_sources[:] = 0.0
    u[:, 3:] = u[:, :1] * conc
    for b in range(len(mesh.boundaries)):
        bv = ref.boundary_values[b]
        bv[:, 0] = np.where(bv[:, 0] < 0.1, 0.0 if dry else 0.5, bv[:, 0])
        bv[:, 3:] = bv[:, :1] * conc
    F = ref.apply(case.dt, u)
    own = mesh.cell_owned_to_local
    wet = u[own, 0] >= case.config.tiny_h
    assert wet.sum() > 50
    speed = np.sqrt(TR.G * u[:, 0].max()) + 12.0
    e = mesh.edge_internal_ids
    scale = (mesh.edge_lengths[e] / np.minimum(mesh.cell_areas[mesh.edge_cell_ids[2 * e]], mesh.cell_areas[mesh.edge_cell_ids[2 * e + 1]])).max()
    T = scale * u[:, 0].max() * speed
    for j in range(2):
        want = conc[j] * F[wet, 0] - 0.001 - 0.01 * conc[j]
        err = np.abs(F[wet, 3 + j] - want).max()
        print(f"riemann={riemann} tracer {j}: max |F - (c F0 - 0.001 - 0.01 c)| = {err:.3e}, T = {T:.3e}")
        assert err <= 1e-12 * max(1.0, T * conc[j])


# ---- the reference's sediment convergence study (driver/tests/sediment/sediment_mms_conv_study.yaml and its upwind twin) ----
CONC = 0.5          # mms.constants.C
# expected_rates of the two files (L1, L2, Linf); the run fails unless every fitted rate EXCEEDS its number (src/rdymms.c:1005)
SEDIMENT_EXPECTED = {
    TR.RIEMANN_ROE: {"h": (0.94, 0.95, 0.94), "hu": (0.91, 0.93, 0.77), "hv": (0.91, 0.93, 0.77), "c0": (0.94, 0.95, 0.94), "c1": (0.93, 0.93, 0.95)},
    TR.RIEMANN_UPWIND_ROE: {"h": (0.94, 0.95, 0.94), "hu": (0.91, 0.93, 0.77), "hv": (0.91, 0.93, 0.77), "c0": (0.94, 0.95, 0.94), "c1": (0.93, 0.92, 0.95)},
}


def sediment_fields(x, y, t):
    """c0, c1 of the yaml's mms.sediment section with their derivatives: (c, dcdx, dcdy, dcdt) per class"""
    s, c, K, T = np.sin, np.cos, mms.K, mms.T
    out = []
    for sign in (1.0, -1.0):
        et = np.exp(sign * t / T)
        out.append((CONC * (1 + s(K * x) * s(K * y)) * et, CONC * K * s(K * y) * c(K * x) * et, CONC * K * s(K * x) * c(K * y) * et,
                    sign * CONC / T * (1 + s(K * x) * s(K * y)) * et))
    return out


def sediment_solution(x, y, t):
    """(h, hu, hv, h c0, h c1): what the solution vector holds (src/rdymms.c:352-440)"""
    flow = mms.solution(x, y, t)
    return np.concatenate([flow] + [flow[:, :1] * f[0][:, None] for f in sediment_fields(x, y, t)], axis=1)


def sediment_sources(x, y, t):
    """the manufactured source of class i (src/rdymms.c:596-628): d(h c)/dt + div(h c u) - (e - d)"""
    d = mms.fields(x, y, t)
    h, u, v = d["h"], d["u"], d["v"]
    Cd = mms.G * d["n"] ** 2 * h ** (-1.0 / 3.0)
    tau_b = 0.5 * TR.RHO_WATER * Cd * (u * u + v * v)
    ei = TR.KP * (tau_b - TR.TAU_EROSION) / TR.TAU_EROSION
    out = []
    for ci, dcdx, dcdy, dcdt in sediment_fields(x, y, t):
        src = ci * d["dhdt"] + h * dcdt
        src += u * ci * d["dhdx"] + h * ci * d["dudx"] + u * h * dcdx
        src += v * ci * d["dhdy"] + h * ci * d["dvdy"] + v * h * dcdy
        di = TR.SETTLING * ci * (1.0 - tau_b / TR.TAU_DEPOSITION)
        out.append(src - (ei - di))
    return np.stack(out, axis=1)


def sediment_run_level(refinements, make_apply, dt=0.01, t_stop=5.0, nsteps=None):
    """mms.run_level for the five components: initial condition and errors at cell centroids, Dirichlet values at edge
    centroids and sources at cell centroids at t + dt/2 before every step, forward Euler"""
    mesh = mms.level_mesh(refinements)
    apply = make_apply(mesh)
    cx, cy = mesh.cell_centroids[:, 0], mesh.cell_centroids[:, 1]
    be = mesh.boundaries[0].edge_ids
    ex, ey = mesh.edge_centroids[be, 0], mesh.edge_centroids[be, 1]
    u = sediment_solution(cx, cy, 0.0)
    t = 0.0
    for _ in range(int(round(t_stop / dt)) if nsteps is None else nsteps):
        th = t + 0.5 * dt
        u = apply(dt, u, mms.source_terms(cx, cy, th), sediment_sources(cx, cy, th), sediment_solution(ex, ey, th))
        t += dt
    err = u - sediment_solution(cx, cy, t)
    a = mesh.cell_areas[:, None]
    return mesh.num_cells, (np.abs(err) * a).sum(axis=0), np.sqrt((err * err * a).sum(axis=0)), np.abs(err).max(axis=0), u


def reference_make_apply(riemann):
    def make_apply(mesh):
        ref = TR.TracerReference(mesh, [M.CONDITION_DIRICHLET], 2, riemann)
        c = mesh.cell_centroids
        ref.mannings[:] = mms.fields(c[:, 0], c[:, 1], 0.0)["n"]

        def apply(dt, u, src, tsrc, bvals):
            ref.external_sources[:] = src
            ref.tracer_sources[:] = tsrc
            ref.boundary_values[0][:] = bvals
            return u + dt * ref.apply(dt, u)
        return apply
    return make_apply


@pytest.mark.parametrize("riemann", [TR.RIEMANN_ROE, TR.RIEMANN_UPWIND_ROE])
def test_sediment_mms_rates_exceed_the_reference_thresholds(riemann):
    """The whole study of the yaml files: base_refinement 1, num_refinements 3 (four levels), dt = 0.01, 500 steps; rates by
    linear regression of log10(error) on log10(num_cells), times -2 (src/rdymms.c:920-1008)."""
    xs, norms = [], []
    for r in range(1, 5):
        n, l1, l2, li, _ = sediment_run_level(r, reference_make_apply(riemann))
        xs.append(np.log10(n))
        norms.append(np.log10(np.stack([l1, l2, li])))
    norms = np.array(norms)                                    # [level, norm, component]
    for ci, comp in enumerate(("h", "hu", "hv", "c0", "c1")):
        for ni, norm in enumerate(("L1", "L2", "Linf")):
            rate = -2.0 * np.polyfit(np.array(xs), norms[:, ni, ci], 1)[0]
            thr = SEDIMENT_EXPECTED[riemann][comp][ni]
            print(f"riemann={riemann} {comp} {norm}: rate {rate:.4f} (threshold {thr})")
            assert np.isfinite(rate) and rate > thr, f"{norm} rate for {comp}: {rate} (expected > {thr})"


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_every_new_entry_point_reports_a_null_operator():
    lib = _lib.load()
    n, r, p, nv = C.c_int32(), C.c_int32(), C.c_void_p(), C.c_int64()
    v = (C.c_double * 8)()
    calls = {
        "rdyhip_tracers_enable": (None, 2, 0),
        "rdyhip_tracers_info": (None, C.byref(n), C.byref(r)),
        "rdyhip_tracers_set_boundary_values": (None, 0, 1, v),
        "rdyhip_tracers_set_source": (None, 0, 1, None, v),
        "rdyhip_tracers_rhs_function": (None, 0.1, None, None, None),
        "rdyhip_tracers_euler_step": (None, 0.1, None, None, None, None),
        "rdyhip_tracers_primitive_variables": (None, C.byref(p), C.byref(nv)),
        "rdyhip_tracers_get_boundary_fluxes": (None, 0, 1, v),
    }
    assert sorted(calls) == sorted(s for s in _lib.SYMBOLS if s.startswith("rdyhip_tracers_"))
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())


def test_every_tracer_kernel_keeps_its_rows_in_registers():
    """2 slot counts x 7 tracer counts x 2 flux variants; a per-thread array that went to scratch, or a spilled register,
    shows in the code object's metadata"""
    res = {k: v for k, v in codeobj.kernel_resources(build.lib_path()).items() if "tracer_rhs_kernel<" in k}
    forms = {k.split("tracer_rhs_kernel<")[1].split(">")[0] for k in res}
    assert forms == {f"{s}, {nt}, {up}" for s in (3, 4) for nt in range(1, 8) for up in ("false", "true")} and len(res) == 28
    bad = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr_spills"] != 0}
    assert not bad, bad
    assert max(v["vgpr"] + v["agpr"] for v in res.values()) <= 256          # at least two waves per SIMD
