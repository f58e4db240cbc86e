"""GPU: the classical Runge-Kutta step behind the C ABI (rdyhip_rk4_step, csrc/rk_kernels.h) against the loop it replaces --
EulerStepper(temporal="rk4", fused=False): four RHS calls, three copies and seven axpy_owned launches per step.  The one-call
step must give that loop's BITS: state (ghost rows included), Courant struct, boundary fluxes, primitive variables; both are
held to the oracle-driven loop (helpers.oracle_rk4) at the 1e-10 of test_rk4_advance_matches_oracle_loop."""
import dataclasses
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from rdycore_amd import build
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import LIMITER_MINMOD, WELL_BALANCING_HR
from helpers import oracle_from_case, oracle_rk4, rel_linf
from test_gpu_c_client import compile_client, write_case

TOL = 1e-10
NSTEPS = 3
EX2B = os.path.join(ROOT, "tests", "golden", "planar_dam_10x5.msh")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _strip_rank(interleaved=False):
    """rank 1 of 3 strips of a 120 x 48 triangle mesh (3840 owned cells, a column of ghosts on either side): ghosts numbered
    behind the owned cells, or -- `interleaved` -- in the source's row-major order, mixed with them (the o2l layout)"""
    K = 2 * np.pi / 37
    z = CS.mms_bathymetry(K=K)
    nxp, ny, rank, world = 40, 48, 1, 3
    if not interleaved:
        mesh = M.strip_partition_tri_mesh(nxp, ny, rank, world, 1.0, zfunc=z)
    else:
        i0, nxl = rank * nxp - 1, nxp + 2
        xyz, conn, cqi, cqj = M.structured_tri_connectivity(nxl, ny, 1.0, i0=i0)
        xyz[:, 2] = z(xyz[:, 0], xyz[:, 1])
        gi = cqi + i0
        owned = (gi >= rank * nxp) & (gi < (rank + 1) * nxp)
        gids = 2 * (cqj.astype(np.int64) * (nxp * world) + gi) + np.arange(conn.shape[0]) % 2
        mesh = M.extract_local_mesh(xyz, conn, owned, cell_global_ids=gids, num_cells_global=2 * nxp * world * ny,
                                    boundary_classifier=M.box_side_boundaries(0.0, nxp * world, 0.0, ny), ghosts="interleaved")
    return CS.friction_slope_case(mesh, nxp * world, ny, dt=1e-2, K=K)


def _quad_part_odd():
    """the left five columns of a 9 x 7 quad mesh with the sixth as ghosts behind them: 35 owned cells (3 * n_owned odd, so the
    16-byte form meets the pair that straddles the end of the owned rows) and 7 ghosts whose rows the stage kernel copies"""
    K = 2 * np.pi / 23
    nx, ny = 9, 7
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    xyz = np.zeros(((nx + 1) * (ny + 1), 3))
    xyz[:, 0], xyz[:, 1] = ii.ravel(), jj.ravel()
    xyz[:, 2] = CS.mms_bathymetry(K=K)(xyz[:, 0], xyz[:, 1])
    qi, qj = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy"))
    v = lambda i, j: j * (nx + 1) + i
    conn = np.stack([v(qi, qj), v(qi + 1, qj), v(qi + 1, qj + 1), v(qi, qj + 1)], 1).astype(np.int32)
    mesh = M.extract_local_mesh(xyz, conn, qi < 5, boundary_classifier=M.box_side_boundaries(0.0, nx, 0.0, ny))
    assert mesh.num_owned_cells == 35 and mesh.num_cells == 42
    return CS.friction_slope_case(mesh, nx, ny, dt=1e-2, K=K, dry_disc=False)


def _case(kind):
    if kind == "quad_part_odd":
        return _quad_part_odd()
    if kind == "ex2b":
        return CS.ex2b_case(EX2B)
    if kind == "quads_15x7":                       # 105 cells: 3 * n_owned is odd, the 16-byte form ends in its scalar tail
        K = 2 * np.pi / 23
        return CS.friction_slope_case(M.structured_quad_mesh(15, 7, 1.0, 1.0, zfunc=CS.mms_bathymetry(K=K)), 15, 7, dt=1e-2, K=K)
    if kind == "tri_40x48":                        # 3840 cells: several workgroups
        K = 2 * np.pi / 37
        return CS.friction_slope_case(M.structured_tri_mesh(40, 48, 1.0, zfunc=CS.mms_bathymetry(K=K)), 40, 48, dt=1e-2, K=K)
    if kind == "strip_rank":
        return _strip_rank()
    if kind == "strip_rank_interleaved":
        return _strip_rank(interleaved=True)
    raise ValueError(kind)


def _configs(case, rdyhip_kernel):
    """(name, case, dt): first order, hydrostatic reconstruction, second order (minmod) -- the last two live in the tiled
    kernels; second order needs its gradient exchange wherever there are ghost cells, i.e. a halo"""
    out = [("first_order", case, case.dt)]
    if rdyhip_kernel != "cell":
        out.append(("hr", dataclasses.replace(case, config=dataclasses.replace(case.config, well_balancing=WELL_BALANCING_HR)), case.dt))
        if case.mesh.num_cells == case.mesh.num_owned_cells:
            cfg = dataclasses.replace(case.config, second_order=True, limiter=LIMITER_MINMOD)
            out.append(("second_order", dataclasses.replace(case, config=cfg), 0.1 * case.dt))
    return out


class _LocalRows:
    """the oracle's RHS as rows of the LOCAL vector (zero in the ghost rows), so that helpers.oracle_rk4's updates advance the
    owned rows and leave the ghost rows alone -- what a rank without a halo does"""

    def __init__(self, orc, mesh):
        self.orc, self.own = orc, np.asarray(mesh.cell_owned_to_local)

    def apply(self, dt, u):
        f = np.zeros_like(u)
        f[self.own] = self.orc.apply(dt, u)
        return f


def _run(op, case, dt, fused, u=None):
    """NSTEPS Runge-Kutta steps; everything a caller can see afterwards"""
    torch = _torch()
    from rdycore_amd.timestep import EulerStepper
    if u is None:
        u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    op.release_primitive_variables()               # the evaluations do not store them: the request below is the first
    st = EulerStepper(op, temporal="rk4", fused=fused)
    st.advance(u, dt, NSTEPS * dt)
    assert st.step == NSTEPS
    pv = op.primitive_variables.clone()
    op.update_diagnostics()
    torch.cuda.synchronize()
    return {"u": u, "pv": pv, "courant": op.get_diagnostics(), "bflux": [op.boundary_fluxes(b) for b in range(len(case.mesh.boundaries))]}


def _assert_same(a, b, what):
    torch = _torch()
    assert torch.equal(a["u"], b["u"]), f"{what}: state"
    assert torch.equal(a["pv"], b["pv"]), f"{what}: primitive variables"
    assert a["courant"] == b["courant"], f"{what}: {a['courant']} / {b['courant']}"
    for x, y in zip(a["bflux"], b["bflux"]):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: boundary fluxes"


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", ["ex2b", "quads_15x7", "tri_40x48", "strip_rank", "strip_rank_interleaved", "quad_part_odd"])
def test_one_call_step_gives_the_bits_of_the_loop_and_matches_the_oracle(kind, rdyhip_kernel):
    torch = _torch()
    base = _case(kind)
    mesh = base.mesh
    for name, case, dt in _configs(base, rdyhip_kernel):
        op = CS.create_operator(case)
        info = op.layout_info()
        assert bool(info["owned_is_prefix"]) == (kind != "strip_rank_interleaved")
        loop = _run(op, case, dt, fused=False)
        step = _run(op, case, dt, fused=True)
        _assert_same(step, loop, f"{kind} {name}")
        assert bool(torch.isfinite(step["u"]).all())
        ghost = torch.as_tensor(np.nonzero(mesh.cell_is_owned == 0)[0], device="cuda")
        assert torch.equal(step["u"][ghost], torch.tensor(case.u_local, device="cuda")[ghost])   # no halo: nobody writes them
        ref = oracle_rk4(_LocalRows(oracle_from_case(case), mesh), case.u_local, dt, NSTEPS)
        err = rel_linf(step["u"].cpu().numpy(), ref)
        print(f"{kind} {name}: rel L-inf vs the oracle loop after {NSTEPS} steps = {err:.3e}")
        assert err <= TOL, (kind, name, err)
        assert rel_linf(ref, case.u_local) > 1e-6          # the state has moved
        if name == "first_order":
            # a state array that starts 8 bytes into its buffer: the 8-byte form of the kernels (with ghosts: of its copy of
            # the ghost rows too), the same bits
            buf = torch.empty(3 * mesh.num_cells + 1, dtype=torch.float64, device="cuda")
            u8 = buf[1:].view(mesh.num_cells, 3)
            assert u8.data_ptr() % 16 == 8 and step["u"].data_ptr() % 16 == 0
            u8.copy_(torch.tensor(case.u_local, dtype=torch.float64))
            _assert_same(_run(op, case, dt, fused=True, u=u8), step, f"{kind} {name}, unaligned state")
        op.destroy()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_workspace_is_allocated_once_and_counted():
    torch = _torch()
    case = _case("strip_rank")
    mesh = case.mesh
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    b0 = op.layout_info()["device_bytes"]
    op.rk4_step(case.dt, u)
    b1 = op.layout_info()["device_bytes"]
    op.rk4_step(case.dt, u)
    b2 = op.layout_info()["device_bytes"]
    torch.cuda.synchronize()
    assert b1 - b0 == (mesh.num_cells + 4 * mesh.num_owned_cells) * 24 and b2 == b1
    # the tensor checks of euler_step
    from rdycore_amd.operator import RDyHipError
    with pytest.raises(RDyHipError):
        op.rk4_step(case.dt, u[:-1])
    with pytest.raises(RDyHipError):
        op.rk4_step(case.dt, u.float())
    # RDYHIP_ERR_USER from the ABI itself: a halo of another operator (one without peers will do), a null state array
    import ctypes as C
    from rdycore_amd import _lib
    lib = _lib.load()
    other = CS.create_operator(case)
    halo = C.c_void_p()
    _lib.check(lib.rdyhip_halo_create(other._h, None, 0, None, None, None, None, None, C.byref(halo)))
    before = u.clone()
    assert lib.rdyhip_rk4_step(op._h, halo, case.dt, u.data_ptr(), None) == 83 and b"another operator" in lib.rdyhip_last_error()
    assert lib.rdyhip_rk4_step(op._h, None, case.dt, None, None) == 83 and b"null u_local" in lib.rdyhip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(u, before)
    assert lib.rdyhip_rk4_step(other._h, halo, case.dt, u.data_ptr(), None) == 0       # its own halo, no peers: no exchange
    torch.cuda.synchronize()
    _lib.check(lib.rdyhip_halo_destroy(C.byref(halo)))
    other.destroy()
    op.destroy()


# ---- three ranks on one GPU (gloo, the bytes through the ABI's transport callback) --------------------------------------------

def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RDYHIP_OVERLAP"] = "1"            # the two-stream form of every step
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rdycore_amd.halo import HaloExchange
        from rdycore_amd.timestep import EulerStepper
        from test_gpu_multirank import _cases
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        case, _, _ = _cases("strips", rank, world, False)
        op = CS.create_operator(case)
        halo = HaloExchange(case.mesh, dev, transport="c", op=op)
        u0 = torch.tensor(case.u_local, dtype=torch.float64, device=dev)
        dts = 0.1 * case.dt
        res = {}
        # two steps, the one-call step against the loop of rhs_overlapped / copy / axpy calls
        ua, ub = u0.clone(), u0.clone()
        EulerStepper(op, halo=halo, temporal="rk4", fused=True).advance(ua, dts, 2 * dts)
        EulerStepper(op, halo=halo, temporal="rk4", fused=False).advance(ub, dts, 2 * dts)
        torch.cuda.synchronize()
        res["step_is_loop"] = bool(torch.equal(ua, ub)) and bool(torch.isfinite(ua).all()) and not bool(torch.equal(ua, u0))
        if os.environ.get("RDYHIP_KERNEL") == "cell":      # the fused pack rides on the tiled Euler-step kernels: nothing more here
            assert halo.fuse_pack(True) is False
            q.put((rank, res))
            halo.destroy()
            op.destroy()
            return

        def advance_step_advance(fuse):
            u = u0.clone()
            st = EulerStepper(op, halo=halo)                  # fused Euler steps: turns the fused pack on
            assert halo.fuse_pack(fuse) is fuse
            st.advance(u, dts, 5 * dts)
            op.rk4_step(dts, u, halo=halo)
            st.advance(u, dts, 5 * dts)
            torch.cuda.synchronize()
            return u

        def steps_step_step(fuse, with_halo):
            """the Euler steps called one by one, so that nothing but rdyhip_rk4_step itself can tell the halo that the rows it
            mirrors in its send buffer have been rewritten: four steps end in `u` with the pack of `u` in the send buffer.
            Without a halo the stages see the ghost rows as they are and no exchange of theirs touches the send buffer: only
            the reset at the head of rdyhip_rk4_step keeps the next Euler step from sending the rows of before."""
            u, u2 = u0.clone(), torch.empty_like(u0)
            assert halo.fuse_pack(fuse) is fuse
            halo.invalidate()
            for _ in range(2):
                halo.step_overlapped(op, dts, u, u2)
                halo.step_overlapped(op, dts, u2, u)
            op.rk4_step(dts, u, halo=halo if with_halo else None)
            halo.step_overlapped(op, dts, u, u2)
            halo.step_overlapped(op, dts, u2, u)             # its exchange brings the rows the neighbours were sent into play
            torch.cuda.synchronize()
            return u

        own = torch.as_tensor(case.mesh.cell_owned_to_local, device=dev).long()
        res["advance_rk4_advance"] = bool(torch.equal(advance_step_advance(True), advance_step_advance(False)))
        for with_halo in (True, False):
            a, b = steps_step_step(True, with_halo), steps_step_step(False, with_halo)
            res[f"steps_rk4_step_halo_{with_halo}"] = bool(torch.equal(a[own], b[own])) and bool(torch.isfinite(a[own]).all())
        q.put((rank, res))
        halo.destroy()
        op.destroy()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(240)
def test_three_ranks_one_gpu(rdyhip_kernel):
    """strips on three ranks, transport="c": the one-call step with its four overlapped stage evaluations = the loop, bit for
    bit on every rank (both kernel variants); and, with the tiled kernels, an rk4_step between fused-pack Euler steps on the same array leaves no stale send rows behind"""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(200)
    for p in procs:
        if p.is_alive():
            p.terminate()
            p.join(10)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for rank, res in sorted(q.get(timeout=5) for _ in range(world)):
        assert all(res.values()), (rank, res)


# ---- the step from a plain C host ------------------------------------------------------------------------------------------------

def test_rk4_client_compiles_as_c11(tmp_path):
    assert os.path.exists(compile_client(tmp_path, "rdyhip_rk4_client"))


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_c_host_takes_rk4_steps_on_ex2b(tmp_path):
    """tests/c_client/rdyhip_rk4_client.c: 40 steps of rdyhip_rk4_step on ex2b = the oracle-driven loop"""
    build.build_native()
    case = CS.ex2b_case(EX2B)
    no = case.mesh.num_owned_cells
    path, out_path = str(tmp_path / "ex2b.bin"), str(tmp_path / "out.bin")
    write_case(path, case, True, np.zeros((no, 3)), np.zeros((no, 3)), np.zeros((no, 3)), 0.0)
    exe = compile_client(tmp_path, "rdyhip_rk4_client")
    env = dict(os.environ)
    env.pop("RDYHIP_LIB", None)
    dt, n = 0.01, 40
    run = subprocess.run([exe, path, out_path, str(n), repr(dt)], capture_output=True, text=True, env=env, timeout=100)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = open(out_path, "rb").read()
    steps, = struct.unpack("q", raw[:8])
    courant, = struct.unpack("d", raw[8:16])
    u_c = np.frombuffer(raw[16:], dtype=np.float64).reshape(-1, 3)
    assert steps == n and courant > 0.0
    ref = oracle_rk4(oracle_from_case(case), case.u_local, dt, n)
    err = rel_linf(u_c, ref)
    print(f"C host, {n} steps: rel L-inf vs the oracle loop = {err:.3e}")
    assert err <= TOL
