"""GPU: the tracer path on several ranks -- the phased evaluations (rdyhip_tracer_phase_*) and the halo object's tracer steps
(rdyhip_halo_tracers_*), in one process: the other ranks are played by a scripted RDyHipTransportFn that knows the undivided
state (tests/tracer_parts.py).  It copies the send buffer aside and fills the receive buffer's per-peer slices with the rows
the owners would send, on the stream it is given; the pack is checked by comparing the copy with the owned rows of the send
lists, the receive by the ghost rows, both bit for bit.

Meshes (the smallest where this can go wrong): one rank's part with ghosts interleaved (972 owned cells: the unpack path, the
owned -> local table, 4 workgroups that each hold both kinds of cell); the three RCB parts of a jittered 24 x 24 triangle mesh
(owned cells first, ghosts grouped by owner: direct receive); a band one row of squares wide (INTERIOR is empty); 30 triangles
with a halo of no peers (HALO is empty); a rank that owns nothing.  NT = 1, 2 and 7, the upwind flux with NT = 2.
tests/test_tracers_multirank_cpu.py checks without a device that every state used here is finite, that its largest Courant
number stands clear of the runner-up and that every mesh has the cells its case needs: no assertion here is conditional.

Bars: bits against rdyhip_tracers_rhs_function / _euler_step on a complete array wherever the same rank's arithmetic is
compared; 1e-10 (helpers.rel_linf, the bar of test_gpu_tracers.py) against tracer_reference.py on the undivided mesh, 1e-12 for
its Courant number, exact ids."""
import ctypes as C
import functools

import numpy as np
import pytest

import tracer_parts as TP
import tracer_reference as TR
from helpers import rel_linf
from rdycore_amd import _lib
from rdycore_amd import cases as CS
from rdycore_amd import mesh as M
from rdycore_amd.operator import Operator, RDyFlowConfig, RDyHipError, _DeviceArray
from test_gpu_tracers import _bits, _dev, _empty_mesh, _torch

pytestmark = pytest.mark.gpu

TOL = 1e-10
SENT = -777.0
ALL, INTERIOR, HALO = 0, 1, 2
RESET = 2                      # RDYHIP_PHASE_RESET_DIAGNOSTICS
KIND_RHS, KIND_EULER = 2, 3    # RDYHIP_HALO_STEP_TRACERS_RHS / _EULER
COMBOS = [(1, TR.RIEMANN_ROE), (2, TR.RIEMANN_UPWIND_ROE), (7, TR.RIEMANN_ROE)]
NAMES = ["part-o2l", "rcb-0", "rcb-1", "rcb-2", "band", "tri-30"]


def _part(name, nt, riemann):
    if name.startswith("rcb-"):
        return TP.rcb(nt, riemann)[5][int(name[4:])]
    return TP.single(name, nt, riemann)


def _arm(op, ref):
    """the tracer path of an existing operator enabled, with every input of the reference set"""
    op.enable_tracers(ref.nt, ref.riemann)
    for j in range(ref.nt):
        op.tracers_set_source(j, ref.tracer_sources[:, j])
    for b, bnd in enumerate(ref.mesh.boundaries):
        if bnd.num_edges:
            op.tracers_set_boundary_values(b, ref.boundary_values[b])
    return op


def _operator(part):
    return _arm(CS.create_operator(part.case), part.ref)


def _full(shape, value):
    return _torch().full(shape, value, dtype=_torch().float64, device="cuda")


def _courant(op):
    op.update_diagnostics()
    d = op.get_diagnostics()
    return (int(_bits(np.array([d.max_courant_num]))[0]), int(d.global_edge_id), int(d.global_cell_id))


def _collect(op, mesh, f, pv, out=None):
    """everything an evaluation leaves behind, as bits"""
    _torch().cuda.synchronize()
    res = {"F": _bits(f.cpu().numpy()), "pv": _bits(pv.cpu().numpy()), "courant": _courant(op)}
    for b, bnd in enumerate(mesh.boundaries):
        res[f"bflux{b}"] = _bits(op.tracers_boundary_fluxes(b))
    if out is not None:
        res["u_out"] = _bits(out.cpu().numpy())
    return res


def _assert_same(got, want, what=""):
    assert sorted(got) == sorted(want)
    for k in want:
        if k == "courant":
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert np.array_equal(got[k], want[k]), (what, k)


def _whole(part, euler):
    """rdyhip_tracers_rhs_function / _euler_step on the complete array, on an operator of its own: the bits every other form
    of the evaluation has to give (u_out: SENT in the ghost rows)"""
    torch = _torch()
    mesh, n = part.mesh, part.u.shape[1]
    op = _operator(part)
    pv = op.tracers_primitive_variables()
    f = _full((mesh.num_owned_cells, n), float("nan"))
    out = _full((mesh.num_cells, n), SENT) if euler else None
    if euler:
        op.tracers_euler_step(part.case.dt, _dev(part.u), out, f)
    else:
        op.tracers_rhs_function(part.case.dt, _dev(part.u), f)
    res = _collect(op, mesh, f, pv, out)
    assert np.isfinite(f.cpu().numpy()).all()
    op.destroy()
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _whole_of(name, nt, riemann, euler):
    """_whole of a named part: computed once, shared (the tracer kernel does not depend on RDYHIP_KERNEL)"""
    res = _whole(_part(name, nt, riemann), euler)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


class Scripted:
    """an RDyHipHalo of `part`'s pattern whose transport is this object: `truth[ncomp]` is the complete local array the ghost
    rows are served from, `sent` the copy of the send buffer of the last exchange"""

    def __init__(self, op, part, recv_ids=None, peers=None):
        torch = _torch()
        self.lib, self.op, self.part = _lib.load(), op, part
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(_lib.c_int32_p)
        self.peers = i32(part.peers if peers is None else peers)
        self.send_ids, self.recv_ids = i32(part.send_ids), i32(part.recv_ids if recv_ids is None else recv_ids)
        self.ns, self.nr = self.send_ids.size, self.recv_ids.size
        self._recv_dev = torch.as_tensor(self.recv_ids.astype(np.int64), device="cuda")
        self.truth, self.sent, self.calls, self.widths = {}, None, 0, []
        self.h = C.c_void_p()
        _lib.check(self.lib.rdyhip_halo_create(op._h, None, len(self.peers), p(self.peers), p(i32(part.send_counts)), p(self.send_ids),
                                               p(i32(part.recv_counts)), p(self.recv_ids), C.byref(self.h)))
        self._cb = _lib.TRANSPORT_FN(self._transport)
        _lib.check(self.lib.rdyhip_halo_set_transport(self.h, C.cast(self._cb, C.c_void_p), None))

    def _transport(self, ctx, d_send, d_recv, ncomp, stream):
        try:
            torch = _torch()
            s = torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream()
            with torch.cuda.stream(s):
                self.calls += 1
                self.widths.append(int(ncomp))
                self.sent = torch.as_tensor(_DeviceArray(d_send, (self.ns * ncomp,), self), device="cuda").clone().view(self.ns, ncomp) if self.ns else None
                if self.nr:
                    dst = torch.as_tensor(_DeviceArray(d_recv, (self.nr * ncomp,), self), device="cuda")
                    dst.copy_(self.truth[int(ncomp)][self._recv_dev].reshape(-1))
            return 0
        except Exception:                       # never let an exception cross the C boundary
            import traceback
            traceback.print_exc()
            return 1

    def serve(self, complete):
        """the complete local array [num_cells, ncomp] the next exchanges of that width are served from"""
        self.truth[int(complete.shape[1])] = _dev(complete)

    def st(self):
        return int(_torch().cuda.current_stream().cuda_stream)

    def rhs(self, dt, u, f):
        _lib.check(self.lib.rdyhip_halo_tracers_rhs(self.op._h, self.h, float(dt), u.data_ptr(), f.data_ptr() if f is not None else None, self.st()))

    def step(self, dt, u, out, f=None):
        _lib.check(self.lib.rdyhip_halo_tracers_euler_step(self.op._h, self.h, float(dt), u.data_ptr(), out.data_ptr(),
                                                           f.data_ptr() if f is not None else None, self.st()))

    def set_form(self, kind, form):
        _lib.check(self.lib.rdyhip_halo_set_form(self.h, kind, form))

    def form_info(self, kind):
        fi = _lib.RDyHipHaloFormInfo()
        _lib.check(self.lib.rdyhip_halo_form_info(self.h, kind, C.byref(fi)))
        return fi

    def as_halo_exchange(self):
        """the rdycore_amd.halo.HaloExchange of a run on three ranks, around this handle (its constructor plans the pattern over
        torch.distributed, which one process does not have)"""
        from rdycore_amd.halo import HaloExchange
        hx = HaloExchange.__new__(HaloExchange)
        hx.transport, hx._halo, hx._comm, hx.world, hx.rank, hx.device = "c", self.h, None, 3, 1, _torch().device("cuda")
        return hx

    def destroy(self):
        _torch().cuda.synchronize()
        _lib.check(self.lib.rdyhip_halo_destroy(C.byref(self.h)))


def _ghosts(mesh):
    return np.nonzero(mesh.cell_is_owned == 0)[0]


def _with_nan_ghosts(part):
    u = np.array(part.u)
    u[_ghosts(part.mesh)] = np.nan
    return _dev(u)


# ---- 1. the phases equal the whole, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,riemann", COMBOS)
@pytest.mark.parametrize("name", NAMES)
def test_interior_then_halo_is_the_whole_evaluation(name, nt, riemann):
    part = _part(name, nt, riemann)
    mesh, dt, n = part.mesh, part.case.dt, 3 + nt
    halo = TP.ghost_adjacent(mesh)
    o2l = np.asarray(mesh.cell_owned_to_local)
    op = _operator(part)
    pv = op.tracers_primitive_variables()
    u = _dev(part.u)
    for euler in (False, True):
        want = _whole_of(name, nt, riemann, euler)
        f = _full((mesh.num_owned_cells, n), SENT)
        out = _full((mesh.num_cells, n), SENT) if euler else None
        pv.fill_(SENT)

        def run(phase, reset):
            if euler:
                op.tracers_euler_step_phase(phase, dt, u, out, f, reset_diagnostics=reset)
            else:
                op.tracers_rhs_phase(phase, dt, u, f, reset_diagnostics=reset)
        run(INTERIOR, True)
        _torch().cuda.synchronize()
        # INTERIOR alone: the rows of the ghost-adjacent cells and all ghost rows are untouched, the others are the whole's
        for arr, key, rows, other in ((f, "F", ~halo, halo), (pv, "pv", ~halo, halo)) + (((out, "u_out", o2l[~halo], np.concatenate([o2l[halo], _ghosts(mesh)])),) if euler else ()):
            a = arr.cpu().numpy()
            assert (a[other] == SENT).all(), (key, "INTERIOR wrote rows of the other phase")
            assert np.array_equal(_bits(a[rows]), want[key][rows]), key
        run(HALO, False)
        _assert_same(_collect(op, mesh, f, pv, out), want, f"{name} euler={euler}")
        # HALO alone (with the reset flag): the rows of the interior cells are untouched
        f.fill_(SENT)
        pv.fill_(SENT)
        if euler:
            out.fill_(SENT)
        run(HALO, True)
        _torch().cuda.synchronize()
        for arr, key, rows, other in ((f, "F", halo, ~halo), (pv, "pv", halo, ~halo)) + (((out, "u_out", o2l[halo], np.concatenate([o2l[~halo], _ghosts(mesh)])),) if euler else ()):
            a = arr.cpu().numpy()
            assert (a[other] == SENT).all(), (key, "HALO wrote rows of the other phase")
            assert np.array_equal(_bits(a[rows]), want[key][rows]), key
        # PHASE_ALL with the reset flag is the unphased call
        run(INTERIOR, True)
        run(ALL, True)
        _assert_same(_collect(op, mesh, f, pv, out), want, f"{name} euler={euler} PHASE_ALL")
    assert np.array_equal(_bits(u.cpu().numpy()), _bits(part.u))
    op.destroy()


# ---- 2. the Courant record merges ----------------------------------------------------------------------------------------------------
def test_the_courant_record_merges_across_the_phases():
    nt, riemann = 2, TR.RIEMANN_UPWIND_ROE
    part = TP.single("part-o2l", nt, riemann)
    mesh, dt = part.mesh, part.case.dt
    halo = TP.ghost_adjacent(mesh)
    op = _operator(part)
    f = _full((mesh.num_owned_cells, 3 + nt), 0.0)
    for k, (state, cell) in enumerate(TP.courant_states(part)):
        u = _dev(state)
        op.tracers_rhs_function(dt, u, f)
        whole = _courant(op)
        c, _ = TP.owned_side_courant(mesh, part.ref, state, dt)
        value = float(np.array([whole[0]], dtype=np.int64).view(np.float64)[0])
        print(f"state {k}: maximum {value:.6f} (numpy {c.max():.6f}), interior {c[~halo].max():.6f}, halo {c[halo].max():.6f}")
        assert abs(value - c.max()) <= 1e-12 * max(1.0, c.max())
        assert halo[int(np.argmax(c))] == (k == 1)                # the maximum is an INTERIOR cell's (state 0), a HALO cell's (state 1)
        op.tracers_rhs_phase(INTERIOR, dt, u, f, reset_diagnostics=True)
        op.tracers_rhs_phase(HALO, dt, u, f)
        assert _courant(op) == whole                              # value bits and ids, wherever the maximum is
        op.tracers_rhs_phase(HALO, dt, u, f)                      # merging twice changes nothing
        assert _courant(op) == whole
        # HALO with the reset flag after INTERIOR: the HALO cells' own maximum -- the flag is honoured
        op.tracers_rhs_phase(INTERIOR, dt, u, f, reset_diagnostics=True)
        op.tracers_rhs_phase(HALO, dt, u, f, reset_diagnostics=True)
        own = _courant(op)
        v = float(np.array([own[0]], dtype=np.int64).view(np.float64)[0])
        assert abs(v - c[halo].max()) <= 1e-12 * max(1.0, c[halo].max())
        if k == 0:
            assert v < value and own != whole
        else:
            assert own == whole
        # and INTERIOR alone reports the interior cells' own
        op.tracers_rhs_phase(INTERIOR, dt, u, f, reset_diagnostics=True)
        vi = float(np.array([_courant(op)[0]], dtype=np.int64).view(np.float64)[0])
        assert abs(vi - c[~halo].max()) <= 1e-12 * max(1.0, c[~halo].max())
    op.destroy()


# ---- 3. overlapped steps, both forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name,nt,riemann", [("part-o2l", 1, TR.RIEMANN_ROE), ("part-o2l", 2, TR.RIEMANN_UPWIND_ROE), ("part-o2l", 7, TR.RIEMANN_ROE),
                                              ("rcb-0", 7, TR.RIEMANN_ROE), ("rcb-1", 2, TR.RIEMANN_UPWIND_ROE), ("rcb-2", 1, TR.RIEMANN_ROE),
                                              ("band", 2, TR.RIEMANN_UPWIND_ROE)])
def test_overlapped_steps_in_both_forms(name, nt, riemann, form):
    torch = _torch()
    part = _part(name, nt, riemann)
    mesh, dt, n = part.mesh, part.case.dt, 3 + nt
    op = _operator(part)
    pv = op.tracers_primitive_variables()
    h = Scripted(op, part)
    h.serve(part.u)
    assert bool(h.lib.rdyhip_halo_direct_receive(h.h)) == (name != "part-o2l")        # ghosts in one run behind the owned cells, or interleaved
    same = lambda x, y: torch.equal(x.view(torch.int64), y.view(torch.int64))         # bits, compared on the device
    complete, sent_want = _dev(part.u), _dev(part.u[part.send_ids])
    start = np.array(part.u)
    start[_ghosts(mesh)] = np.nan
    for euler, kind in ((False, KIND_RHS), (True, KIND_EULER)):
        want = _whole_of(name, nt, riemann, euler)
        want_dev = {k: _dev(want[k].view(np.float64)) for k in ("F", "pv") + (("u_out",) if euler else ())}
        h.set_form(kind, form)
        fi = h.form_info(kind)
        assert (fi.form, fi.source) == (form, 2)

        def once(what):
            u = _dev(start)
            f = _full((mesh.num_owned_cells, n), float("nan"))
            out = _full((mesh.num_cells, n), SENT) if euler else None
            pv.fill_(SENT)
            calls = h.calls
            if euler:
                h.step(dt, u, out, f)
            else:
                h.rhs(dt, u, f)
            assert _courant(op) == want["courant"], what
            assert h.calls == calls + 1 and h.widths[-1] == n
            assert same(u, complete), (what, "ghost rows are the owners' rows, owned rows as they were")
            assert same(h.sent, sent_want), (what, "the pack")
            assert same(f, want_dev["F"]) and same(pv, want_dev["pv"]), what
            assert not euler or same(out, want_dev["u_out"]), (what, "u_out: owned rows, SENT in the ghost rows")
            for b in range(len(mesh.boundaries)):
                assert np.array_equal(_bits(op.tracers_boundary_fluxes(b)), want[f"bflux{b}"]), what
        for i in range(3):                                             # events and buffers are reused
            once(f"{name} euler={euler} form={form} call {i}")
        # the trial: 16 steps alternate between the forms, the next call reads the timings; the same bits throughout
        h.set_form(kind, -1)
        assert h.form_info(kind).source == 0
        for i in range(17):
            once(f"{name} euler={euler} trial step {i}")
        fi = h.form_info(kind)
        assert fi.trial_steps == 16 and fi.source in (1, 3), (fi.trial_steps, fi.source)
    h.destroy()
    op.destroy()
    torch.cuda.synchronize()


# ---- 4. against the reference across ranks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("nt,riemann", COMBOS)
def test_three_parts_against_the_reference_on_the_undivided_mesh(nt, riemann, form):
    g_mesh, case, ref, u, F, parts = TP.rcb(nt, riemann)
    got = np.full_like(F, np.nan)
    best = (0.0, -1, -1)
    for part in parts:
        mesh = part.mesh
        op = _operator(part)
        h = Scripted(op, part)
        h.serve(part.u)
        h.set_form(KIND_RHS, form)
        f = _full((mesh.num_owned_cells, 3 + nt), float("nan"))
        ud = _with_nan_ghosts(part)
        h.rhs(case.dt, ud, f)
        _torch().cuda.synchronize()
        assert np.array_equal(_bits(ud.cpu().numpy()), _bits(part.u))
        got[np.asarray(mesh.cell_global_ids)[mesh.cell_owned_to_local]] = f.cpu().numpy()
        op.update_diagnostics()
        d = op.get_diagnostics()
        if d.max_courant_num > best[0]:                               # timestep.reduce_courant: a later rank replaces on a strictly larger value
            best = (d.max_courant_num, int(d.global_edge_id), int(d.global_cell_id))
        h.destroy()
        op.destroy()
    err = rel_linf(got, F)
    print(f"nt={nt} riemann={riemann} form={form}: F of the three parts vs the undivided reference {err:.3e}")
    assert np.isfinite(got).all() and err <= TOL
    cmax, edge, cell = ref.courant
    assert abs(best[0] - cmax) <= 1e-12 * max(1.0, cmax)
    # the parts number their edges by the global vertex pair, the undivided mesh by position: compare the vertex pairs
    assert best[1] == int(TP.edge_keys(g_mesh)[edge])
    assert best[2] == int(g_mesh.cell_global_ids[cell])


# ---- 5. a halo sized before the tracers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rcb-1", "part-o2l"])
def test_a_halo_created_before_the_tracers_grows_its_buffers(name):
    torch = _torch()
    nt, riemann = 7, TR.RIEMANN_ROE
    part = _part(name, nt, riemann)
    mesh, dt, n = part.mesh, part.case.dt, 3 + nt
    lib = _lib.load()
    want = _whole_of(name, nt, riemann, False)
    op = CS.create_operator(part.case)
    h = Scripted(op, part)                                             # sized for 3 values per cell
    h.serve(part.u)
    h.serve(part.u[:, :3])
    u3 = np.array(part.u[:, :3])
    u3[_ghosts(mesh)] = np.nan

    def swe():
        f3 = _full((mesh.num_owned_cells, 3), float("nan"))
        ud = _dev(u3)
        _lib.check(lib.rdyhip_rhs_overlapped(op._h, h.h, dt, ud.data_ptr(), f3.data_ptr(), h.st()))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(ud.cpu().numpy()), _bits(part.u[:, :3]))
        return _bits(f3.cpu().numpy()), _courant(op)
    before = swe()
    wide = _with_nan_ghosts(part)
    assert lib.rdyhip_halo_exchange(h.h, wide.data_ptr(), n, h.st()) != 0       # 3-wide buffers still
    with pytest.raises(RDyHipError) as e:                                        # tracers not enabled yet
        h.rhs(dt, wide, _full((mesh.num_owned_cells, n), 0.0))
    assert e.value.code == 83 and "not enabled" in e.value.message
    _arm(op, part.ref)
    pv = op.tracers_primitive_variables()
    f = _full((mesh.num_owned_cells, n), float("nan"))
    h.rhs(dt, wide, f)                                                           # the first tracer step grows the buffers
    got = _collect(op, mesh, f, pv)
    _assert_same(got, want, "first tracer step on a halo sized for 3")
    assert np.array_equal(_bits(wide.cpu().numpy()), _bits(part.u)) and np.array_equal(_bits(h.sent.cpu().numpy()), _bits(part.u[part.send_ids]))
    after = swe()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(_bits(h.sent.cpu().numpy()), _bits(part.u[part.send_ids, :3]))
    wide = _with_nan_ghosts(part)
    _lib.check(lib.rdyhip_halo_exchange(h.h, wide.data_ptr(), n, h.st()))       # works from then on
    torch.cuda.synchronize()
    assert np.array_equal(_bits(wide.cpu().numpy()), _bits(part.u))
    h.destroy()
    op.destroy()


def test_a_tracer_step_between_two_fused_pack_steps(monkeypatch):
    """tiled kernel, halo created before the tracers: euler_step_overlapped, a tracer step (which grows the send buffer the fused
    pack's lists point into, and leaves 3 + NT-wide rows there), euler_step_overlapped on the first step's output -- the same
    bits as without the fused pack, and the second step's exchange sends the rows of ITS input"""
    torch = _torch()
    monkeypatch.setenv("RDYHIP_KERNEL", "tiled")
    nt, riemann = 7, TR.RIEMANN_ROE
    part = _part("rcb-1", nt, riemann)
    mesh, dt, n = part.mesh, part.case.dt, 3 + nt
    lib = _lib.load()
    ghosts = _ghosts(mesh)
    runs = []
    for fuse in (0, 1):
        op = CS.create_operator(part.case)
        assert op.layout_info()["tiled_kernel"] == 1
        h = Scripted(op, part)
        _lib.check(lib.rdyhip_halo_fuse_pack(h.h, fuse))
        assert lib.rdyhip_halo_pack_fused(h.h) == fuse
        _arm(op, part.ref)
        h.serve(part.u)
        h.serve(part.u[:, :3])
        u3 = np.array(part.u[:, :3])
        u3[ghosts] = np.nan
        a, b, c = _dev(u3), _full((mesh.num_cells, 3), SENT), _full((mesh.num_cells, 3), SENT)
        _lib.check(lib.rdyhip_euler_step_overlapped(op._h, h.h, dt, a.data_ptr(), b.data_ptr(), None, h.st()))
        f, wide = _full((mesh.num_owned_cells, n), float("nan")), _with_nan_ghosts(part)
        h.rhs(dt, wide, f)
        torch.cuda.synchronize()
        assert h.widths[-1] == n and np.array_equal(_bits(h.sent.cpu().numpy()), _bits(part.u[part.send_ids]))
        _lib.check(lib.rdyhip_euler_step_overlapped(op._h, h.h, dt, b.data_ptr(), c.data_ptr(), None, h.st()))
        torch.cuda.synchronize()
        bn, cn = b.cpu().numpy(), c.cpu().numpy()
        assert h.widths[-1] == 3 and np.array_equal(_bits(h.sent.cpu().numpy()), _bits(bn[part.send_ids])), "the second step sent stale rows"
        assert np.array_equal(_bits(bn[ghosts]), _bits(part.u[ghosts, :3])) and (cn[ghosts] == SENT).all()
        runs.append((_bits(bn), _bits(cn), _bits(f.cpu().numpy()), _courant(op)))
        h.destroy()
        op.destroy()
    for x, y in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(x, y)
    assert runs[0][3] == runs[1][3]
    assert (runs[0][1].view(np.float64)[np.asarray(mesh.cell_owned_to_local)] != SENT).all()      # every owned row of the second step was written


# ---- 6. TracerEulerStepper ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sediment_reference(riemann):
    """the reference loop on the undivided mesh, once: (mesh, per step (dt, state before, flow source, tracer source, Dirichlet
    values), final state)"""
    from test_tracers_cpu import reference_make_apply, sediment_run_level
    steps, holder = [], {}

    def recording(mesh):
        holder["mesh"] = mesh
        inner = reference_make_apply(riemann)(mesh)

        def apply(dt, u, src, tsrc, bvals):
            steps.append((dt, np.array(u), np.array(src), np.array(tsrc), np.array(bvals)))
            return inner(dt, u, src, tsrc, bvals)
        return apply
    _, _, _, _, want = sediment_run_level(1, recording, nsteps=40)
    assert len(steps) == 40
    return holder["mesh"], steps, want


@pytest.mark.parametrize("form", [0, 1])
def test_tracer_euler_stepper_on_one_part_of_the_sediment_mms_case(form):
    """40 steps of the reference's sediment MMS case on part 1 of a three-part RCB cut, every step one
    HaloExchange.tracers_step_overlapped with the sources and Dirichlet values of its half time; the ghost rows come from the
    reference loop on the undivided mesh, which is also what the owned rows are compared with"""
    import mms
    from rdycore_amd import partition as P
    from rdycore_amd.timestep import TracerEulerStepper
    torch = _torch()
    riemann = TR.RIEMANN_ROE
    g, steps, want = _sediment_reference(riemann)
    c = g.cell_centroids
    g_ref = TR.TracerReference(g, [M.CONDITION_DIRICHLET], 2, riemann)
    g_ref.mannings[:] = mms.fields(c[:, 0], c[:, 1], 0.0)["n"]
    dt, u0 = steps[0][0], steps[0][1]
    g_case = CS.Case("sediment", g, RDyFlowConfig(), [M.CONDITION_DIRICHLET], u0[:, :3], g_ref.mannings, np.zeros((g.num_cells, 3)), {}, dt)
    part = TP.split(g, g_case, g_ref, u0, 3, P.owned_cell_boundaries())[1]
    mesh = part.mesh
    gid = np.asarray(mesh.cell_global_ids)
    own = gid[mesh.cell_owned_to_local]
    op = CS.create_operator(part.case)
    op.enable_tracers(2, riemann)
    h = Scripted(op, part)
    h.set_form(KIND_EULER, form)
    stepper = TracerEulerStepper(op, halo=h.as_halo_exchange())
    start = np.array(u0[gid])
    start[_ghosts(mesh)] = np.nan
    cur = _dev(start)
    for k, (dt, u_k, src, tsrc, bvals) in enumerate(steps):
        for comp in range(3):
            op.set_domain_external_source(comp, src[own, comp])
        for j in range(2):
            op.tracers_set_source(j, tsrc[own, j])
        op.tracers_set_boundary_values(0, bvals[part.bpos[0]])
        h.serve(u_k[gid])
        cur = stepper.advance(cur, dt, 1)
    torch.cuda.synchronize()
    assert stepper.step == 40 and h.calls == 40
    got = cur.cpu().numpy()[mesh.cell_owned_to_local]
    err = float(np.abs(got - want[own]).max() / np.abs(want).max())     # relative to the state's own size (h ~ 0.005), as test_gpu_tracers.py
    print(f"form={form}: part 1 of 3, {mesh.num_owned_cells} owned cells, 40 steps, state vs the undivided reference {err:.3e}")
    assert np.isfinite(got).all() and err <= TOL
    # without a halo the stepper is rdyhip_tracers_euler_step: one step on the complete array gives the bits of the halo step
    for comp in range(3):
        op.set_domain_external_source(comp, steps[0][2][own, comp])
    for j in range(2):
        op.tracers_set_source(j, steps[0][3][own, j])
    op.tracers_set_boundary_values(0, steps[0][4][part.bpos[0]])
    h.serve(u0[gid])
    a = TracerEulerStepper(op, halo=h.as_halo_exchange()).advance(_dev(start), dt, 1).cpu().numpy()
    b = TracerEulerStepper(op).advance(_dev(u0[gid]), dt, 1).cpu().numpy()
    assert np.array_equal(_bits(a[mesh.cell_owned_to_local]), _bits(b[mesh.cell_owned_to_local]))
    h.destroy()
    op.destroy()


# ---- 7. argument errors and edge cases -------------------------------------------------------------------------------------------------
def test_refusals():
    torch = _torch()
    lib = _lib.load()
    nt, riemann = 2, TR.RIEMANN_UPWIND_ROE
    part = TP.single("part-o2l", nt, riemann)
    mesh, n = part.mesh, 3 + nt
    plain = CS.create_operator(part.case)                              # tracers not enabled
    op = _operator(part)
    h, hp = Scripted(op, part), Scripted(plain, part)
    u, out = _dev(part.u), _full((mesh.num_cells, n), SENT)
    f = _full((mesh.num_owned_cells, n), SENT)
    up, op_, fp, st = u.data_ptr(), out.data_ptr(), f.data_ptr(), h.st()

    def refused(rc, text):
        assert rc == 83 and text in lib.rdyhip_last_error().decode(), (rc, lib.rdyhip_last_error())
    refused(lib.rdyhip_halo_tracers_rhs(op._h, None, 0.1, up, fp, st), "null halo")
    refused(lib.rdyhip_halo_tracers_euler_step(op._h, None, 0.1, up, op_, None, st), "null halo")
    refused(lib.rdyhip_tracer_phase_rhs(plain._h, 0, 2, 0.1, up, fp, st), "not enabled")
    refused(lib.rdyhip_tracer_phase_euler_step(plain._h, 0, 2, 0.1, up, op_, None, st), "not enabled")
    refused(lib.rdyhip_halo_tracers_rhs(plain._h, hp.h, 0.1, up, fp, st), "not enabled")
    refused(lib.rdyhip_halo_tracers_rhs(op._h, hp.h, 0.1, up, fp, st), "another operator")
    refused(lib.rdyhip_halo_tracers_euler_step(op._h, hp.h, 0.1, up, op_, None, st), "another operator")
    refused(lib.rdyhip_tracer_phase_rhs(op._h, 0, 2, 0.1, None, fp, st), "null u_local")
    refused(lib.rdyhip_tracer_phase_rhs(op._h, 0, 2, 0.1, up, None, st), "f_global")
    refused(lib.rdyhip_tracer_phase_euler_step(op._h, 0, 2, 0.1, None, op_, None, st), "null u_local")
    refused(lib.rdyhip_halo_tracers_rhs(op._h, h.h, 0.1, None, fp, st), "null u_local")
    refused(lib.rdyhip_halo_tracers_rhs(op._h, h.h, 0.1, up, None, st), "f_global")
    refused(lib.rdyhip_halo_tracers_euler_step(op._h, h.h, 0.1, None, op_, None, st), "null u_local")
    refused(lib.rdyhip_tracer_phase_euler_step(op._h, 0, 2, 0.1, up, up, None, st), "not in place")
    refused(lib.rdyhip_tracer_phase_euler_step(op._h, 0, 2, 0.1, up, None, None, st), "not in place")
    refused(lib.rdyhip_halo_tracers_euler_step(op._h, h.h, 0.1, up, up, None, st), "not in place")
    refused(lib.rdyhip_halo_tracers_euler_step(op._h, h.h, 0.1, up, None, None, st), "not in place")
    for phase in (3, -1):
        refused(lib.rdyhip_tracer_phase_rhs(op._h, phase, 2, 0.1, up, fp, st), "unknown phase")
        refused(lib.rdyhip_tracer_phase_euler_step(op._h, phase, 2, 0.1, up, op_, None, st), "unknown phase")
    for flags in (4, 8, 2 | 16, -1):
        refused(lib.rdyhip_tracer_phase_rhs(op._h, 0, flags, 0.1, up, fp, st), "unknown flags")
        refused(lib.rdyhip_tracer_phase_euler_step(op._h, 0, flags, 0.1, up, op_, None, st), "unknown flags")
    for kind in (4, -1):
        assert lib.rdyhip_halo_set_form(h.h, kind, 0) == 83 and lib.rdyhip_halo_form_info(h.h, kind, C.byref(_lib.RDyHipHaloFormInfo())) == 83
    torch.cuda.synchronize()
    assert h.calls == 0 and hp.calls == 0                              # refused before any exchange ...
    assert (f.cpu().numpy() == SENT).all() and (out.cpu().numpy() == SENT).all()   # ... and before any launch
    # RDYHIP_PHASE_OVERWRITE is implied and accepted
    _lib.check(lib.rdyhip_tracer_phase_rhs(op._h, 0, 1 | 2, 0.1, up, fp, st))
    for x in (h, hp):
        x.destroy()
    for x in (op, plain):
        x.destroy()


def test_the_tracer_kinds_stay_in_order_where_two_streams_cannot_work():
    nt, riemann = 2, TR.RIEMANN_UPWIND_ROE
    # a receive list that names an owned row: rdyhip_halo_create locks the halo in order
    part = TP.single("part-o2l", nt, riemann)
    op = _operator(part)
    recv = np.array(part.recv_ids)
    recv[0] = part.mesh.cell_owned_to_local[5]
    h = Scripted(op, part, recv_ids=recv)
    for kind in (KIND_RHS, KIND_EULER):
        for form in (1, -1, 1):
            h.set_form(kind, form)
            fi = h.form_info(kind)
            assert (fi.form, fi.source) == (0, 4)
    h.destroy()
    op.destroy()
    # a halo without peers: HALO is empty, nothing travels, the step is the whole evaluation
    part = TP.single("tri-30", nt, riemann)
    mesh, n = part.mesh, 3 + nt
    assert not part.peers
    op = _operator(part)
    pv = op.tracers_primitive_variables()
    h = Scripted(op, part)
    for euler, kind in ((False, KIND_RHS), (True, KIND_EULER)):
        want = _whole_of("tri-30", nt, riemann, euler)
        h.set_form(kind, 1)
        fi = h.form_info(kind)
        assert (fi.form, fi.source) == (0, 4)
        f, out = _full((mesh.num_owned_cells, n), float("nan")), (_full((mesh.num_cells, n), SENT) if euler else None)
        pv.fill_(SENT)
        if euler:
            h.step(part.case.dt, _dev(part.u), out, f)
        else:
            h.rhs(part.case.dt, _dev(part.u), f)
        _assert_same(_collect(op, mesh, f, pv, out), want)
    assert h.calls == 0
    h.set_form(0, 1)                                                   # the SWE kinds are forced as before
    assert (h.form_info(0).form, h.form_info(0).source) == (1, 2)
    h.destroy()
    op.destroy()


def test_a_rank_that_owns_nothing_still_takes_part_in_the_exchange():
    torch = _torch()
    mesh = _empty_mesh()
    nt, n = 3, 6
    op = Operator.create(RDyFlowConfig(), mesh)
    op.enable_tracers(nt)
    truth = np.random.default_rng(3).uniform(0.1, 1.0, (mesh.num_cells, n))
    z = np.zeros(0, dtype=np.int32)
    part = TP.Part(mesh, None, None, truth, [1], np.array([0], dtype=np.int32), z, np.array([mesh.num_cells], dtype=np.int32),
                   np.arange(mesh.num_cells, dtype=np.int32))
    h = Scripted(op, part)
    h.serve(truth)
    f = torch.empty((0, n), dtype=torch.float64, device="cuda")
    for form in (0, 1):
        for euler, kind in ((False, KIND_RHS), (True, KIND_EULER)):
            h.set_form(kind, form)
            u, out = _full((mesh.num_cells, n), float("nan")), _full((mesh.num_cells, n), SENT)
            calls = h.calls
            if euler:
                h.step(0.1, u, out)
            else:
                h.rhs(0.1, u, f)
            torch.cuda.synchronize()
            assert h.calls == calls + 1 and h.sent is None
            assert np.array_equal(_bits(u.cpu().numpy()), _bits(truth)) and (out.cpu().numpy() == SENT).all()
            op.update_diagnostics()
            assert op.get_diagnostics().max_courant_num == 0.0
    for phase in (ALL, INTERIOR, HALO):
        op.tracers_rhs_phase(phase, 0.1, _dev(truth), f, reset_diagnostics=True)
        op.tracers_euler_step_phase(phase, 0.1, _dev(truth), _full((mesh.num_cells, n), SENT))
    h.destroy()
    op.destroy()


@pytest.mark.parametrize("name", ["part-o2l", "rcb-2"])
def test_the_swe_path_is_undisturbed(name):
    """rdyhip_rhs_overlapped on an operator with tracers, after tracer steps of both forms on the same halo, gives the bits of a
    fresh operator with a fresh halo: F, primitive variables, boundary fluxes, the Courant struct"""
    torch = _torch()
    lib = _lib.load()
    nt, riemann = 2, TR.RIEMANN_UPWIND_ROE
    part = _part(name, nt, riemann)
    mesh, dt, n = part.mesh, part.case.dt, 3 + nt
    plain, op = CS.create_operator(part.case), _operator(part)
    hp, h = Scripted(plain, part), Scripted(op, part)
    h.serve(part.u)
    for form in (0, 1):
        h.set_form(KIND_RHS, form)
        h.set_form(KIND_EULER, form)
        ud, fd, od = _with_nan_ghosts(part), _full((mesh.num_owned_cells, n), 0.0), _full((mesh.num_cells, n), 0.0)
        h.rhs(dt, ud, fd)
        h.step(dt, ud, od)
        torch.cuda.synchronize()
    u3 = np.array(part.u[:, :3])
    u3[_ghosts(mesh)] = np.nan
    res = []
    for o, x in ((plain, hp), (op, h)):
        x.serve(part.u[:, :3])
        x.set_form(0, 1)
        pv = o.primitive_variables
        f = _full((mesh.num_owned_cells, 3), float("nan"))
        ud = _dev(u3)
        _lib.check(lib.rdyhip_rhs_overlapped(o._h, x.h, dt, ud.data_ptr(), f.data_ptr(), x.st()))
        torch.cuda.synchronize()
        o.update_diagnostics()
        d = o.get_diagnostics()
        res.append(([_bits(f.cpu().numpy()), _bits(pv.cpu().numpy()), _bits(ud.cpu().numpy()), _bits(x.sent.cpu().numpy())] +
                    [_bits(o.boundary_fluxes(b)) for b in range(len(mesh.boundaries))], (d.max_courant_num, d.global_edge_id, d.global_cell_id)))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert res[0][1] == res[1][1] and res[0][1][0] > 0.0
    assert np.isfinite(res[0][0][0].view(np.float64)).all()
    for x in (h, hp):
        x.destroy()
    for o in (op, plain):
        o.destroy()
