"""GPU parity on randomised inputs: irregular triangle meshes (jittered vertices, random
diagonals), random bathymetry, states that sit on every branch of the arithmetic -- dry and
nearly-dry cells around tiny_h, supercritical and transcritical jumps (the Roe entropy fix,
src/swe/swe_roe_flux_petsc.h:56-67), inflow through critical-outflow edges, ANUGA velocity
regularisation (h_anuga_regular > 0) -- for both friction methods, first and second order and
hydrostatic reconstruction.  Tolerance 1e-10 as everywhere."""
import os

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig

from helpers import oracle_from_case, rel_linf
from random_cases import random_case, random_tri_mesh
from test_gpu_parity import check_all, run_both

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.mark.parametrize("seed", range(int(os.environ.get("RDYHIP_FUZZ_SEEDS", "6"))))   # RDYHIP_FUZZ_SEEDS=200: a longer soak
@pytest.mark.parametrize("variant", ["first", "second_minmod", "second_vanleer", "second_none", "hr"])
def test_random_meshes_and_states(seed, variant, rdyhip_kernel):
    if rdyhip_kernel == "cell" and variant != "first":
        pytest.skip("tiled kernels only")
    rng = np.random.default_rng(1000 + seed)
    cfg = RDyFlowConfig(tiny_h=float(rng.choice([1e-7, 1e-5])), h_anuga_regular=float(rng.choice([0.0, 0.0, 1e-3])),
                        source_method=int(seed % 2))
    if variant.startswith("second"):
        cfg.second_order = True
        cfg.limiter = {"second_minmod": 0, "second_none": 1, "second_vanleer": 2}[variant]
    if variant == "hr":
        cfg.well_balancing = 2
    scale = int(os.environ.get("RDYHIP_FUZZ_SCALE", "1"))    # larger meshes for a soak run (many tiles per mesh)
    mesh = random_tri_mesh(rng, scale * int(rng.integers(9, 30)), scale * int(rng.integers(7, 22)), project_2d=(variant == "hr"))
    case = random_case(rng, mesh, cfg)
    f, fr, op, orc = run_both(case)
    assert np.isfinite(fr).all()
    check_all(case, f, fr, op, orc)


def test_entropy_fix_branch_is_exercised():
    # a transcritical rarefaction across every interior edge: |lambda| < d(lambda) triggers the critical-flow fix
    from oracle import oracle as O
    hits = 0
    rng = np.random.default_rng(5)
    for _ in range(200):
        hl, hr = rng.uniform(0.5, 2.0), rng.uniform(0.05, 0.4)
        ul = rng.uniform(0.0, 2.0)
        ur = ul + rng.uniform(3.0, 6.0)
        cl, cr, chat = np.sqrt(9.806 * hl), np.sqrt(9.806 * hr), np.sqrt(0.5 * 9.806 * (hl + hr))
        uhat = (np.sqrt(hl) * ul + np.sqrt(hr) * ur) / (np.sqrt(hl) + np.sqrt(hr))
        hits += abs(uhat - chat) < max(0.0, 2 * ((ur - cr) - (ul - cl)))
    assert hits > 20          # the generator of test_transcritical_edges below lands in the branch
    assert O.roe_flux(1.0, 0.5, 0.0, 0.2, 4.5, 0.0, 0.0, 1.0)[1] > 0.0


def test_transcritical_edges(rdyhip_kernel):
    rng = np.random.default_rng(9)
    mesh = random_tri_mesh(rng, 24, 16)
    xc = mesh.cell_centroids[:, 0]
    # depth falls and velocity rises along x in steps: every x-facing edge is a strong rarefaction
    step = np.floor(xc / 1.5)
    h = 2.0 * 0.75 ** step
    uvel = 0.5 + 1.6 * step
    u = np.stack([h, h * uvel, h * 0.1 * rng.normal(size=h.size)], axis=1)
    case = CS.Case("transcritical", mesh, RDyFlowConfig(), [M.CONDITION_REFLECTING] * len(mesh.boundaries), u,
                   np.full(mesh.num_cells, 0.02), np.zeros((mesh.num_cells, 3)), {}, 1e-3)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    if rdyhip_kernel == "cell":
        return
    case.config.second_order = True
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
