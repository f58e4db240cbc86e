"""Phase 2 of the first-order / HR tiled kernels reads LDS in one batch: the S wave speeds, the 3 S fluxes and the lane's own
side entries are issued together ahead of the slot loop, an empty slot reads the last record's entry of its plane, and the
Courant tie path takes the batch's wave speeds.  The guards, the sums and their order are what they were, so nothing may change
a bit.

The expected values are the bits of the commit before the batch: tools/record_cell_sum_golden.py ran the groups below on that
commit's library and left, under tests/golden/cell_sum_parent/, the SHA-256 of every array (F, u_out, pv, fdiv) -- and the
array itself where it has at most 256 rows -- with the Courant struct.  Every evaluation here is compared with them bit for bit
and held to the oracle (rel L-inf <= 1e-10 against max(1, |ref|), the bar of test_gpu_parity.py, with the oracle's edge and
cell ids).  Each case runs the table family and, with streamed_normals=True, the streamed one.

The groups, the smallest shapes that reach every path of the batch:
  small   8 and 400 triangles (one and two tiles; a dry disc: wet cells with one, two and three dry-dry edges; Dirichlet,
          critical-outflow and reflecting edges), first order, HR, XQ2018, and HR over a bed step on 400 triangles;
          rhs_function, apply onto an f of random rows and rows of -0.0, euler_step with F, with pv, without F with fdiv
  quads   7 020 quads on eight workgroups, the 20 quads + 96 triangles of the mixed mesh (empty fourth slots, 16-bit
          references), a 16 x 15 block of quads: one tile of 511 records, the highest reference next to the draw word
  ties    the two flat pools on 2 400 renumbered triangles: every tile runs the tie path
  walks   17 000 triangles (175 tiles in eight XCD ranges of 22): eight workgroups under both RDYHIP_TILE_WALK values, and the
          dynamic walk on 176, 88, 64 and 48 workgroups -- 1, 2, 2-3 and 3-4 tiles per workgroup: no draw, a first draw, draws
          beyond the range; five launches back to back on one operator (the counters and the LDS word start clean)
  part    an RCB part with o2l and ghosts, in one call and as INTERIOR + HALO (the skipping walk, the list launches)"""
import dataclasses
import functools
import hashlib
import os

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig

from helpers import oracle_from_case, rel_linf
from test_gpu_cell_family_numbering import _uniform_case
import test_gpu_tile_loop_addressing as TL
import test_gpu_uniform_fields as UF

pytestmark = pytest.mark.gpu
TOL = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_sum_parent")
GROUPS = ["small", "quads", "ties", "walks", "part"]
FULL_ROWS = 256          # arrays of at most this many rows are kept whole beside their digest
ARRAYS = ("F", "u_out", "pv", "fdiv")
FORMS = [("rhs", "plain"), ("apply", "plain"), ("euler", "plain"), ("euler", "pv"), ("euler_no_f", "fdiv")]
FAMILIES = ("table", "streamed")


@pytest.fixture(autouse=True)
def _tiled_kernels_only(rdyhip_kernel):
    if rdyhip_kernel == "cell":
        pytest.skip("a test of the tiled kernels (RDYHIP_KERNEL)")


class OsEnv:
    """monkeypatch's setenv / delenv on os.environ, for the recording script"""
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def _family(case, family):
    return case if family == "table" else dataclasses.replace(case, config=dataclasses.replace(case.config, streamed_normals=True))


def _minus_zero_rows(f0):
    f0 = f0.copy()
    f0[::3] = -0.0      # rows a guard must skip, not add +0.0 to
    return f0


# ---- the cases: (case, f0, environment) by name, built once ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _named(name):
    if "/" in name:                                           # "<mesh of test_gpu_tile_loop_addressing>/<operator>"
        mesh_name, operator = name.split("/")
        case, f0 = TL._case(mesh_name, operator)
        return case, _minus_zero_rows(f0), dict(TL.ENV[mesh_name])
    rng = np.random.default_rng(len(name))
    zf = CS.mms_bathymetry(K=TL.K)
    if name == "hr_bed_step":                                 # a step of 0.3 across x = 10: the reconstruction cuts both sides
        mesh = M.structured_tri_mesh(20, 10, 1.0, zfunc=lambda x, y: zf(x, y) + 0.3 * (x > 10.0), project_2d=True)
        case = CS.friction_slope_case(mesh, 20.0, 10.0, dt=1e-2, K=TL.K)
        case.config = RDyFlowConfig(well_balancing=2)
    elif name == "quad16x15":
        mesh = M.structured_quad_mesh(16, 15, 1.0, 1.0, zfunc=zf)
        case = CS.friction_slope_case(mesh, 16.0, 15.0, dt=1e-2, K=TL.K)
        case.config = RDyFlowConfig()
    elif name == "mixed":
        case = CS.mixed_elements_case(os.path.join(os.path.dirname(GOLDEN), "mixed"))
        return case, _minus_zero_rows(rng.normal(size=(case.mesh.num_owned_cells, 3))), {}
    else:
        assert name == "pools"
        case = _uniform_case("tri-small", "pools", 1e-3)
        return case, np.zeros((case.mesh.num_owned_cells, 3)), {}
    case.mannings = np.full(case.mesh.num_owned_cells, 0.015)
    return case, _minus_zero_rows(rng.normal(size=(case.mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0])), {}


@functools.lru_cache(maxsize=None)
def _oracle(name, accumulate):
    """(F, pv, fdiv, Courant) of the oracle: once per case, shared, left unchanged"""
    case, f0, _ = _named(name)
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local, f0.copy() if accumulate else None)
    assert np.isfinite(fr).all()
    out = (fr.copy(), orc.primitive_variables.copy(), orc.flux_divergence.copy(), tuple(orc.diagnostics()))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def check_oracle(name, call, res, what):
    case, _, _ = _named(name)
    fr, pvr, fdr, cref = _oracle(name, call == "apply")
    own = case.mesh.cell_owned_to_local
    refs = {"F": fr, "u_out": case.u_local[own] + case.dt * fr, "pv": pvr, "fdiv": fdr}
    for k in ARRAYS:
        if res[k] is not None:
            err = rel_linf(res[k][own] if k == "u_out" else res[k], refs[k])
            print(f"{what}: {k} rel L-inf vs oracle {err:.3e}")
            assert err <= TOL, (what, k, err)
    c = res["courant"]
    assert abs(c[0] - cref[0]) <= 1e-12 * max(1.0, cref[0]) and c[1:] == tuple(cref[1:]), (what, c, cref)


def _phased(case, call, f0):
    """INTERIOR then HALO launches on one operator, in the result form of test_gpu_tile_loop_addressing._evaluate"""
    op = CS.create_operator(case)
    f, out, c = UF._evaluate(op, case, call, True, f0)
    op.destroy()
    return {"F": f, "u_out": out, "pv": None, "fdiv": None, "courant": c}


def _repeated(case, n):
    """n rhs_function launches back to back on ONE operator, each into a buffer of its own, one wait behind the last"""
    torch = TL._torch()
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    fs = [torch.full((case.mesh.num_owned_cells, 3), 777.0, dtype=torch.float64, device="cuda") for _ in range(n)]
    for f in fs:
        op.rhs_function(case.dt, u, f)
    torch.cuda.synchronize()
    op.update_diagnostics()
    d = op.get_diagnostics()
    res = [{"F": f.cpu().numpy(), "u_out": None, "pv": None, "fdiv": None, "courant": (d.max_courant_num, d.global_edge_id, d.global_cell_id)}
           for f in fs]
    op.destroy()
    return res


def _layout(case, env, setter):
    TL._set_env(setter, env)
    op = CS.create_operator(case)
    info = op.layout_info()
    op.destroy()
    return info


def run_group(group, setter):
    """every evaluation of a group: key -> (case name, call, result).  `setter` is monkeypatch or OsEnv."""
    out = {}

    def forms(name, which, env_extra=None, tag=""):
        case, f0, env = _named(name)
        for fam in FAMILIES:
            for call, want in which:
                TL._set_env(setter, {**env, **(env_extra or {})})
                out[f"{name} {tag}{call} {want} {fam}"] = (name, call, TL._evaluate(_family(case, fam), f0, call, want))

    if group == "small":
        info = {n: _layout(_named(n)[0], {}, setter) for n in ("tri8/first", "tri400/first")}
        assert info["tri8/first"]["num_tiles"] == 1 and info["tri400/first"]["num_tiles"] == 2
        h = _named("tri400/first")[0].u_local[:, 0]
        assert (h == 0).any() and (h > 0).any()                                                # the dry disc
        assert np.ptp(_named("hr_bed_step")[0].mesh.cell_zc) > 0.3
        for name in [f"{m}/{o}" for m in ("tri8", "tri400") for o in TL.OPERATORS] + ["hr_bed_step"]:
            forms(name, FORMS)
    elif group == "quads":
        info = _layout(_named("quad16x15")[0], {}, setter)
        assert info["num_tiles"] == 1 and info["num_edge_records"] == 511 and info["slots_per_cell"] == 4, info
        info = _layout(_named("mixed")[0], {}, setter)
        assert info["slots_per_cell"] == 4 and (_named("mixed")[0].mesh.cell_nverts == 3).any()
        for name in ("quad7020_flat/first", "mixed", "quad16x15"):
            forms(name, FORMS[:2] + FORMS[3:4])
    elif group == "ties":
        forms("pools", [("rhs", "plain"), ("euler", "plain")])
    elif group == "walks":
        info = _layout(_named("tri17000/first")[0], TL.ENV["tri17000"], setter)
        assert info["num_tiles"] == 175 and info["persistent_grid"] == 8
        for walk in ("static", "dynamic"):
            for operator in ("first", "hr"):
                forms(f"tri17000/{operator}", FORMS[:2], {"RDYHIP_TILE_WALK": walk}, f"{walk} 8 ")
        for grid in ("176", "88", "64", "48"):
            forms("tri17000/first", FORMS[:2], {"RDYHIP_TILE_WALK": "dynamic", "RDYHIP_PGRID": grid}, f"dynamic {grid} ")
        case, _, env = _named("tri17000/first")
        for fam in FAMILIES:
            TL._set_env(setter, {**env, "RDYHIP_TILE_WALK": "dynamic"})
            for k, r in enumerate(_repeated(_family(case, fam), 5)):
                out[f"tri17000/first dynamic 8 launch {k} {fam}"] = ("tri17000/first", "rhs", r)
    else:
        assert group == "part"
        for operator in ("first", "hr"):
            name = f"rcb_part/{operator}"
            case, f0, env = _named(name)
            assert case.mesh.num_cells > case.mesh.num_owned_cells and _layout(case, env, setter)["owned_is_prefix"] == 0
            forms(name, FORMS[:3])
            for fam in FAMILIES:
                for call in ("rhs", "apply", "euler"):
                    TL._set_env(setter, env)
                    out[f"{name} phased {call} {fam}"] = (name, call, _phased(_family(case, fam), call, f0))
    return out


# ---- the recorded bits -------------------------------------------------------------------------------------------------------
def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def golden_arrays(results):
    """what the recording script stores for a group's results"""
    g = {}
    for key, (_, _, res) in results.items():
        for k in ARRAYS:
            if res[k] is not None:
                g[f"{key}|{k}|sha256"] = _digest(res[k])
                if res[k].shape[0] <= FULL_ROWS:
                    g[f"{key}|{k}|full"] = res[k]
        g[f"{key}|courant_max"] = np.array([res["courant"][0]], dtype=np.float64)
        g[f"{key}|courant_ids"] = np.array(res["courant"][1:], dtype=np.int64)
    return g


@pytest.mark.parametrize("group", GROUPS)
def test_the_batched_cell_sum_gives_the_bits_of_the_commit_before_it_and_the_oracles_values(group, monkeypatch):
    results = run_group(group, monkeypatch)
    with np.load(os.path.join(GOLDEN, group + ".npz")) as z:
        gold = {k: z[k] for k in z.files}
    got = golden_arrays(results)
    assert set(got) == set(gold), sorted(set(got) ^ set(gold))[:10]
    for key, (name, call, res) in results.items():
        for k in ARRAYS:
            if res[k] is None:
                continue
            full = gold.get(f"{key}|{k}|full")
            if full is not None:
                assert np.array_equal(res[k].view(np.uint64), full.view(np.uint64)), \
                    f"{key}: {k} differs from the recorded bits, first at row {np.nonzero((res[k].view(np.uint64) != full.view(np.uint64)).any(axis=1))[0][:5]}"
            assert np.array_equal(got[f"{key}|{k}|sha256"], gold[f"{key}|{k}|sha256"]), f"{key}: {k} differs from the recorded bits"
        assert got[f"{key}|courant_max"].view(np.uint64) == gold[f"{key}|courant_max"].view(np.uint64), (key, res["courant"])
        assert np.array_equal(got[f"{key}|courant_ids"], gold[f"{key}|courant_ids"]), (key, res["courant"])
        check_oracle(name, call, res, key)
    if group == "walks":
        for fam in FAMILIES:
            first = results[f"tri17000/first dynamic 8 launch 0 {fam}"][2]
            for k in range(1, 5):
                TL._same_bits(first, results[f"tri17000/first dynamic 8 launch {k} {fam}"][2], f"launch {k} / launch 0, {fam}")
            TL._same_bits(first, results[f"tri17000/first dynamic 8 rhs plain {fam}"][2], f"launch 0 / a new operator's, {fam}")
