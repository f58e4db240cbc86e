"""The water-source plane: while every momentum source is known to be +0.0, the first-order / HR tiled kernels read the
water source from a dense [owned] mirror of component 0 instead of the [owned][3] array (KernelArgs::src_mom, include/rdyhip.h
"the water-source plane").

Meshes of a few thousand cells (test_gpu_kernel_matrix.matrix_mesh) cut into 64-cell tiles on a persistent grid of 8
workgroups: every workgroup walks several tiles, so both call sites of load_streams (the prologue and the pipelined one) run
and the last tile is partial; on the o2l mesh the owned index is not the local one.  The water source differs in every cell.
Tolerance: the bar of test_gpu_parity.py, rel L-inf <= 1e-10 against max(1, |ref|); the two modes of the kernel must agree
bit for bit."""
import ctypes as C

import numpy as np
import pytest

from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd.operator import RDyFlowConfig, _ptr, _stream

from helpers import oracle_from_case, rel_linf
from random_cases import random_case
from test_gpu_kernel_matrix import matrix_mesh
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

MESHES = [("tri", "prefix"), ("quad", "prefix"), ("tri", "o2l")]
_WALK_ENV = {"RDYHIP_TILE_CELLS": "64", "RDYHIP_PGRID": "8"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _walk_env(monkeypatch, kernel=None):
    for k in ("RDYHIP_PGRID", "RDYHIP_XCD_SWIZZLE", "RDYHIP_BALANCE_ROUNDS", "RDYHIP_INTERIOR_SHRINK", "RDYHIP_TILE_CELLS",
              "RDYHIP_UOUT_CACHED", "RDYHIP_BLOCKS_PER_CU", "RDYHIP_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _WALK_ENV.items():
        monkeypatch.setenv(k, v)
    if kernel:
        monkeypatch.setenv("RDYHIP_KERNEL", kernel)


def _case(kind, layout, hr, seed, second_order=False):
    """a random case whose momentum sources are zero (what every shipped workload has) and whose water source differs in
    every cell"""
    rng = np.random.default_rng(seed)
    mesh = matrix_mesh(kind, layout, hr)
    cfg = RDyFlowConfig(tiny_h=1e-5, source_method=int(rng.integers(0, 2)), well_balancing=2 if hr else 0, second_order=second_order)
    case = random_case(rng, mesh, cfg, region_block=64)
    case.dt = 1e-2
    case.ext_src[:, 1:] = 0.0
    assert np.unique(case.ext_src[:, 0]).size == mesh.num_owned_cells
    return rng, case


class Pair:
    """the operator and the oracle of one case, evaluated side by side"""

    def __init__(self, case, rng):
        torch = _torch()
        self.case, self.mesh = case, case.mesh
        self.no = case.mesh.num_owned_cells
        self.op = CS.create_operator(case)
        self.orc = oracle_from_case(case)
        self.ext = case.ext_src.copy()                 # what the source holds now: the oracle's copy follows it
        self.u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
        self.f0 = rng.normal(size=(self.no, 3)) * np.array([0.1, 1.0, 1.0])

    def device(self):
        """rhs_function, the accumulate form and euler_step: (F, pv, F accumulated, u_out, F of the step) as device tensors"""
        torch = _torch()
        op, dt, u = self.op, self.case.dt, self.u
        f = torch.full((self.no, 3), 777.0, dtype=torch.float64, device="cuda")
        op.rhs_function(dt, u, f)
        pv = op.primitive_variables.clone()
        fa = torch.tensor(self.f0, dtype=torch.float64, device="cuda")
        op.reset_diagnostics()
        op.apply(dt, u, fa)
        out = torch.full_like(u, -7.0)
        fe = torch.full((self.no, 3), 777.0, dtype=torch.float64, device="cuda")
        op.euler_step(dt, u, out, fe)
        torch.cuda.synchronize()
        return f, pv, fa, out, fe

    def check(self, what):
        """the three calls against the oracle holding self.ext; returns the device results"""
        case, own = self.case, self.mesh.cell_owned_to_local
        self.orc.external_sources[:] = self.ext
        fr = self.orc.apply(case.dt, case.u_local).copy()
        pvr = self.orc.primitive_variables.copy()
        far = self.orc.apply(case.dt, case.u_local, self.f0.copy())
        assert np.isfinite(fr).all()
        res = self.device()
        f, pv, fa, out, fe = (t.cpu().numpy() for t in res)
        for name, got, ref in (("F", f, fr), ("pv", pv, pvr), ("F accumulated", fa, far), ("F of the Euler step", fe, fr),
                               ("u_out", out[own], case.u_local[own] + case.dt * fr)):
            err = rel_linf(got, ref)
            print(f"{what}: {name}: rel L-inf {err:.3e}")
            assert err <= TOL, f"{what}: {name}: rel L-inf {err:.3e}"
        assert np.all(out[self.mesh.cell_is_owned == 0] == -7.0), "ghost rows of u_out were written"
        return res


def _write_water(p, writer, rng):
    """new water-source values through one of the five writers; p.ext follows"""
    torch = _torch()
    op, no, L = p.op, p.no, _lib.load()
    if writer == "setter_subset":
        ids = rng.permutation(no)[:max(1, no // 3)].astype(np.int32)
        vals = rng.normal(size=ids.size) * 1e-4
        op.set_regional_external_source(ids, 0, vals)
        p.ext[ids, 0] = vals
    elif writer == "setter_on_domain":
        vals = rng.normal(size=no) * 1e-4
        op.set_domain_external_source(0, vals, ordered=True)
        p.ext[:, 0] = vals
    elif writer == "forcing_fill":
        ids = np.sort(rng.permutation(no)[:max(1, no // 5)]).astype(np.int32)
        d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
        _lib.check(L.rdyhip_forcing_fill_source(op._h, 0, ids.size, _ptr(d_ids), 3.25e-5, _stream()))
        p.ext[ids, 0] = 3.25e-5
    elif writer == "forcing_gather":
        data = rng.normal(size=(no + 7, 3)) * 1e-4           # an unstructured dataset: stride 3, offset 2
        dmap = rng.integers(0, no + 7, no).astype(np.int32)
        d_data = torch.tensor(data, dtype=torch.float64, device="cuda")
        d_map = torch.tensor(dmap, dtype=torch.int32, device="cuda")
        _lib.check(L.rdyhip_forcing_gather_source(op._h, 0, no, None, _ptr(d_data), _ptr(d_map), 3, 2, 1.0, _stream()))
        torch.cuda.synchronize()
        p.ext[:, 0] = data[dmap, 2]
    elif writer == "refresh_host":
        p.ext[:, 0] = rng.normal(size=no) * 1e-4
        op.refresh_field(1, p.ext)
    else:
        raise AssertionError(writer)


WRITERS = ["setter_subset", "setter_on_domain", "forcing_fill", "forcing_gather", "refresh_host"]


@pytest.mark.parametrize("hr", [False, True], ids=["plain", "hr"])
@pytest.mark.parametrize("kind,layout", MESHES, ids=[f"{k}-{l}" for k, l in MESHES])
def test_plane_mode_against_the_oracle_and_bit_for_bit_against_the_row_mode(kind, layout, hr, monkeypatch):
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case(kind, layout, hr, 7100 + 10 * MESHES.index((kind, layout)) + int(hr))
    p = Pair(case, rng)
    info = p.op.layout_info()
    assert info["tiled_kernel"] and info["persistent_grid"] == 8 and info["num_tiles"] >= 24     # several tiles per workgroup
    assert info["owned_is_prefix"] == (layout == "prefix")
    assert p.op.source_is_water_only()                    # create_operator set the momentum components from zero arrays
    p.check("after create")
    res = None
    for w in WRITERS:
        _write_water(p, w, rng)
        assert p.op.source_is_water_only(), w
        res = p.check(w)
    # the same calls on the [owned][3] array: reading the field hands out a writable pointer, which ends the plane mode
    ext_dev = p.op.external_sources
    assert not p.op.source_is_water_only()
    assert np.array_equal(ext_dev.cpu().numpy(), p.ext), "the [owned][3] array was not kept current beside the plane"
    rows = p.device()
    for name, a, b in zip(("F", "pv", "F accumulated", "u_out", "F of the Euler step"), res, rows):
        assert torch.equal(a, b), f"{name}: the plane mode and the row mode differ"
    p.op.destroy()


def test_transitions_of_the_mode(monkeypatch):
    torch = _torch()
    _walk_env(monkeypatch)
    rng, case = _case("tri", "o2l", False, 7200)
    p = Pair(case, rng)
    op, no = p.op, p.no
    assert op.source_is_water_only()
    # a momentum source on a few cells, by id: the rows are read from here on
    ids = rng.permutation(no)[:5].astype(np.int32)
    vals = rng.normal(size=5) * 1e-3
    op.set_regional_external_source(ids, 1, vals)
    p.ext[ids, 1] = vals
    assert not op.source_is_water_only()
    p.check("x-momentum source on five cells")
    # water written while the mode is off goes to the rows alone ...
    _write_water(p, "setter_on_domain", rng)
    assert not op.source_is_water_only()
    p.check("water by setter, row mode")
    # ... so that the way back, a host array without momentum sources, has to rewrite the whole plane
    p.ext[:, 0] = rng.normal(size=no) * 1e-4
    p.ext[:, 1:] = 0.0
    op.refresh_field(1, p.ext)
    assert op.source_is_water_only()
    p.check("host refresh_field without momentum: plane rewritten")
    # -0.0 is not +0.0
    op.set_domain_external_source(1, np.zeros(no))
    assert op.source_is_water_only()
    op.set_domain_external_source(2, np.full(no, -0.0), ordered=True)
    assert not op.source_is_water_only()
    op.refresh_field(1, p.ext)
    assert op.source_is_water_only()
    _lib.check(_lib.load().rdyhip_forcing_fill_source(op._h, 2, no, None, 0.0, _stream()))
    assert op.source_is_water_only()
    _lib.check(_lib.load().rdyhip_forcing_fill_source(op._h, 2, no, None, float("nan"), _stream()))
    assert not op.source_is_water_only()
    op.refresh_field(1, p.ext)
    assert op.source_is_water_only()
    # a device array cannot be looked at without blocking
    op.refresh_field(1, torch.tensor(p.ext, dtype=torch.float64, device="cuda"))
    assert not op.source_is_water_only()
    p.check("device refresh_field: row mode")
    op.refresh_field(1, p.ext)
    assert op.source_is_water_only()
    # the const pointer is the same array and leaves the mode alone
    ptr, n = C.c_void_p(), C.c_int64()
    _lib.check(_lib.load().rdyhip_field_ptr_const(op._h, 1, C.byref(ptr), C.byref(n)))
    assert n.value == 3 * no and op.source_is_water_only()
    # the writable one ends it for good
    assert op.external_sources.data_ptr() == ptr.value
    assert not op.source_is_water_only()
    op.refresh_field(1, p.ext)
    assert not op.source_is_water_only()
    p.check("after the escape")
    op.destroy()


@pytest.mark.parametrize("which", ["second_order", "cell"])
def test_second_order_and_cell_kernels_read_the_rows(which, monkeypatch):
    """these kernels always get the [owned][3] array, which the setters keep current while the mode flag is on"""
    _walk_env(monkeypatch, kernel="cell" if which == "cell" else None)
    rng, case = _case("tri", "prefix", False, 7300 + (which == "cell"), second_order=which == "second_order")
    p = Pair(case, rng)
    info = p.op.layout_info()
    assert info["tiled_kernel"] == (which != "cell")
    _write_water(p, "setter_on_domain", rng)
    _write_water(p, "forcing_fill", rng)
    assert p.op.source_is_water_only()
    p.check(which)
    p.op.destroy()
