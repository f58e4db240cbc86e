"""GPU: the output calls of the three states -- rdyhip_state_* / _error_sums / _output_mean_* / _series_* of the SWE state, their
rdyhip_tracer_* counterparts (NT = 2) and their rdyhip_ens_* counterparts (B = 3) -- walked through one fixed script of calls by
ctypes: every refusal (null operator, feature not enabled, mask, form, member, size, null pointers, state machine of the reads,
variables without an accumulator or without time, series not enabled / enabled twice / full / read outside the log) and the
successful paths between them.  Of every call the script keeps the return code and rdyhip_last_error() VERBATIM, of the successful
ones the numbers they deliver as bit patterns (results of more than 32 values as the SHA-256 of those); the whole list must equal tests/golden/output_refusals_parent.json, which
tools/record_output_refusals.py recorded with the same script on the library before the three states' copies of the host code
were folded into shared helpers.  The other output tests match fragments of the messages only.

Mesh: the 44 quads of planar_dam_10x5.msh, once as they are and once with six ghost cells among them (owned cells not a prefix of
the local numbering: every kernel goes through the owned-to-local table, and so do the sites of the series) and the edges in an
order of their own (mesh.dmplex_like_numbering).  No call of the script launches anything it has not checked."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from rdycore_amd import _lib
from rdycore_amd import mesh as M
from rdycore_amd.operator import Operator, RDyFlowConfig

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MSH = os.path.join(HERE, "golden", "planar_dam_10x5.msh")
GOLDEN = os.path.join(HERE, "golden", "output_refusals_parent.json")
NUMBERINGS = ("natural", "o2l")
GHOSTS = (3, 10, 11, 27, 40, 43)
DP, IP = _lib.c_double_p, _lib.c_int32_p


def make_mesh(numbering):
    xyz, conn, _, edge_tag, names = M.read_gmsh41(MSH)
    classify = M.boundaries_from_edge_tags(edge_tag, names)
    if numbering == "natural":
        mesh = M.build_mesh(xyz, conn, boundary_classifier=classify)
        assert mesh.num_owned_cells == mesh.num_cells == 44
        return mesh
    owned = np.ones(conn.shape[0], dtype=np.int32)
    owned[list(GHOSTS)] = 0
    mesh = M.dmplex_like_numbering(M.build_mesh(xyz, conn, is_owned=owned, boundary_classifier=classify), seed=36, hilbert=False)
    assert mesh.num_owned_cells == 38 and (np.asarray(mesh.cell_owned_to_local) != np.arange(38)).any()
    return mesh


HEX_VALUES = 32     # longer results are kept as the SHA-256 of their hex text (tools/record_cell_sum_golden.py does the same)


def digest(text):
    """a result's hex text as the fixture keeps it"""
    return text if len(text) <= 16 * HEX_VALUES else f"sha256 of {len(text) // 16} values: {hashlib.sha256(text.encode()).hexdigest()}"


def hexbits(a):
    return digest("".join(format(int(x), "016x") for x in np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)))


class Walk:
    """calls through ctypes, one record each: the entry point, its return code, rdyhip_last_error() after the call, and what `result`
    gives of a call that returned 0; the labels, which say what a call is there for, are kept beside the records"""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.log, self.labels = [], []
        self.st = int(torch.cuda.current_stream().cuda_stream)

    def __call__(self, label, name, *args, result=None):
        rc = getattr(self.lib, name)(*args)
        err = self.lib.rdyhip_last_error()
        rec = {"call": name, "rc": int(rc), "error": err.decode() if err else ""}
        if result is not None and rc == 0:
            self.torch.cuda.synchronize()
            rec["result"] = result()
        self.log.append(rec)
        self.labels.append(label)
        return rc

    def dev(self, a):
        return self.torch.tensor(np.ascontiguousarray(a), dtype=self.torch.float64, device="cuda")


class Swe:
    """the entry points of one state and the order of their arguments; W values per row, B members"""
    fn, W, B, top = "rdyhip_", 3, 1, 8

    def __init__(self, w, op, rng):
        self.w, self.op, self.h = w, op, op._h
        self.no, self.nc = op.mesh.num_owned_cells, op.mesh.num_cells
        self.un = self.state(rng)
        self.u = w.dev(self.un)

    def state(self, rng):
        u = rng.uniform(-1.0, 1.0, self.shape())
        u[..., 0] = 0.5 + np.abs(u[..., 0])
        u[..., 3:] = u[..., 3:] * u[..., :1]
        u[..., 5, :] = 0.0                       # a dry cell
        return u

    def shape(self):
        return (self.nc, self.W)

    def ptr(self, t):
        return None if t is None else int(t.data_ptr())

    def times(self):
        return (C.c_double * self.B)()

    # argument lists
    def planes(self, h, comps, u, out, form=0):
        return (h, comps, self.ptr(u), self.ptr(out), self.w.st)

    def begin(self, h, comps, u, form=0):
        return (h, comps, self.ptr(u), self.w.st)

    def get(self, h, comp, size, values, member=0):
        return (h, comp, size, values)

    def getptr(self, h, comp, out, member=0):
        return (h, comp, out)

    def accumulate(self, h, vars, dt, us, up):
        return (h, vars, C.c_double(0.5 if dt is None else dt), self.ptr(us), self.w.st)

    def series(self, what, h, *args):
        """(name, arguments) of a series call"""
        kind = 1
        if what == "enable":
            return self.fn + "series_observations_enable", (h,) + args
        if what == "record":
            time, u = args
            return self.fn + "series_record", (h, kind, C.c_double(time), self.ptr(u), self.w.st)
        if what == "info":
            return self.fn + "series_info", (h, kind) + args + (None,)
        if what == "read":
            return self.fn + "series_read", (h, kind) + args + (self.w.st,)
        return self.fn + "series_clear", (h, kind)


class Tracer(Swe):
    fn, W, B, top = "rdyhip_tracer_", 5, 1, 32

    def planes(self, h, comps, u, out, form=0):
        return (h, comps, form, self.ptr(u), self.ptr(out), self.w.st)

    def begin(self, h, comps, u, form=0):
        return (h, comps, form, self.ptr(u), self.w.st)

    def accumulate(self, h, vars, dt, us, up):
        return (h, vars, C.c_double(0.5 if dt is None else dt), self.ptr(us), self.ptr(up), self.w.st)

    def series(self, what, h, *args):
        if what == "record":
            time, u = args
            return self.fn + "series_record", (h, C.c_double(time), self.ptr(u), self.w.st)
        if what == "read":
            return self.fn + "series_read", (h,) + args + (self.w.st,)
        return self.fn + "series_" + what, (h,) + args


class Ens(Tracer):
    fn, W, B, top = "rdyhip_ens_", 3, 3, 8

    def shape(self):
        return (self.B, self.nc, self.W)

    planes, begin = Swe.planes, Swe.begin

    def get(self, h, comp, size, values, member=0):
        return (h, member, comp, size, values)

    def getptr(self, h, comp, out, member=0):
        return (h, member, comp, out)

    def accumulate(self, h, vars, dt, us, up):
        if dt is None:
            dts = None
        elif dt == "one member at 0":
            dts = (C.c_double * self.B)(0.5, 0.0, 0.25)
        else:
            dts = (C.c_double * self.B)(*[dt * (1.0 + 0.25 * m) for m in range(self.B)])
        return (h, vars, dts, self.ptr(us), self.ptr(up), self.w.st)

    def series(self, what, h, *args):
        if what == "record":
            time, u = args
            times = None if time is None else (C.c_double * self.B)(*[time + 0.125 * m for m in range(self.B)])
            return self.fn + "series_record", (h, times, self.ptr(u), self.w.st)
        return Tracer.series(self, what, h, *args)


def walk_readout(w, s, h):
    """the read-out of state `s` through handle `h` (None, an operator without the feature, or the state's own)"""
    f, no, W, torch = s.fn, s.no, s.W, w.torch
    vals = np.full(no, -1.0)
    vp = vals.ctypes.data_as(DP)
    pin = DP()
    ready = C.c_int32(-1)
    out = torch.zeros((s.B * W, no), dtype=torch.float64, device="cuda")
    members = range(s.B)

    def got():
        return hexbits(vals)

    w("before any begin", f + "state_read_get", *s.get(h, 1, no, vp))
    w("before any begin", f + "state_read_ptr", *s.getptr(h, 1, C.byref(pin)))
    w("before any begin", f + "state_read_ready", h, C.byref(ready))
    w("before any begin", f + "state_read_wait", h)
    w("null ready", f + "state_read_ready", h, None)
    for comps in (0, -1, s.top, 1 << 20):
        w(f"mask {comps}", f + "state_planes", *s.planes(h, comps, s.u, out))
        w(f"mask {comps}", f + "state_read_begin", *s.begin(h, comps, s.u))
    w("unknown form", f + "state_planes", *s.planes(h, 1, s.u, out, form=7))
    w("unknown form", f + "state_read_begin", *s.begin(h, 1, s.u, form=-1))
    w("null u", f + "state_planes", *s.planes(h, 1, None, out))
    w("null planes", f + "state_planes", *s.planes(h, 1, s.u, None))
    w("null u", f + "state_read_begin", *s.begin(h, 5, None))
    w("mask 6", f + "state_planes", *s.planes(h, 6, s.u, out), result=lambda: hexbits(out.cpu().numpy()[: 2 * s.B]))
    w("mask top - 1, form 1", f + "state_planes", *s.planes(h, s.top - 1, s.u, out, form=1), result=lambda: hexbits(out.cpu().numpy()))
    # begin -> get before wait -> wait -> get
    w("mask 5", f + "state_read_begin", *s.begin(h, 5, s.u))
    w("before wait", f + "state_read_get", *s.get(h, 1, no, vp))
    w("before wait", f + "state_read_ptr", *s.getptr(h, 4, C.byref(pin)))
    w("in flight", f + "state_read_ready", h, C.byref(ready))          # the answer depends on the clock: not kept
    w("mask 5", f + "state_read_wait", h)
    w("landed", f + "state_read_ready", h, C.byref(ready), result=lambda: ready.value)
    w("landed twice", f + "state_read_wait", h)
    for m in members:
        w(f"member {m} comp 1", f + "state_read_get", *s.get(h, 1, no, vp, m), result=got)
        w(f"member {m} comp 4", f + "state_read_ptr", *s.getptr(h, 4, C.byref(pin), m), result=lambda: hexbits(np.ctypeslib.as_array(pin, (no,))))
    w("comp 2 not asked for", f + "state_read_get", *s.get(h, 2, no, vp))
    w("comp 2 not asked for", f + "state_read_ptr", *s.getptr(h, 2, C.byref(pin)))
    for comp in (3, 5, 0, s.top, -4):
        w(f"comp {comp}", f + "state_read_get", *s.get(h, comp, no, vp))
        w(f"comp {comp}", f + "state_read_ptr", *s.getptr(h, comp, C.byref(pin)))
    for size in (no - 1, no + 1, 0, -1):
        w(f"size {size}", f + "state_read_get", *s.get(h, 1, size, vp))
    w("null values", f + "state_read_get", *s.get(h, 1, no, None))
    w("null pointer", f + "state_read_ptr", *s.getptr(h, 1, None))
    for m in (-1, s.B, s.B + 7):
        w(f"member {m}", f + "state_read_get", *s.get(h, 1, no, vp, m))
        w(f"member {m}", f + "state_read_ptr", *s.getptr(h, 1, C.byref(pin), m))
    # a wider mask (the planes grow), given up for a later begin; a refused begin leaves the landed read alone
    w("mask top - 1: the planes grow", f + "state_read_begin", *s.begin(h, s.top - 1, s.u, form=1))
    w("mask 2 over a read in flight", f + "state_read_begin", *s.begin(h, 2, s.u))
    w("mask 2", f + "state_read_wait", h)
    w("mask 0 after a landed read", f + "state_read_begin", *s.begin(h, 0, s.u))
    w("comp 2", f + "state_read_get", *s.get(h, 2, no, vp, s.B - 1), result=got)
    w("comp 1 not asked for", f + "state_read_get", *s.get(h, 1, no, vp, s.B - 1))


def walk_sums(w, s, h):
    f = s.fn
    sums = (C.c_double * ((3 * 10 + 1) if s.W == 5 else 10 * s.B))()          # RDyHipTracerErrorSums, or B RDyHipErrorSums
    out = C.cast(sums, getattr(w.lib, f + "error_sums_get").argtypes[1])
    exact = w.dev(s.un[..., np.asarray(s.op.mesh.cell_owned_to_local), :] * 0.75 + 0.125)

    def get(label, keep=True):
        w(label, f + "error_sums_get", h, out, result=(lambda: hexbits(np.array(sums[:]))) if keep else None)

    get("before any call", keep=False)
    w("null out", f + "error_sums_get", h, None)
    w("null u", f + "error_sums", h, None, None, w.st)
    w("no exact", f + "error_sums", h, s.ptr(s.u), None, w.st)
    w("null out after a call", f + "error_sums_get", h, None)
    get("no exact")
    get("no exact, again")
    w("exact", f + "error_sums", h, s.ptr(s.u), s.ptr(exact), w.st)
    w("no exact, behind a call in flight", f + "error_sums", h, s.ptr(s.u), None, w.st)
    get("the later call's")
    w("exact", f + "error_sums", h, s.ptr(s.u), s.ptr(exact), w.st)
    get("exact")


def walk_means(w, s, h):
    f, no, W, B, torch = s.fn, s.no, s.W, s.B, w.torch
    mean = torch.zeros(B * no * W + 1, dtype=torch.float64, device="cuda")
    t = s.times()

    def means(off=0):
        return lambda: {"mean": hexbits(mean.cpu().numpy()[off:off + B * no * W]), "time": hexbits(np.array(t[:]))}

    def each(label, vars_list, null_state=False):
        for v in vars_list:
            w(f"{label}: vars {v}", f + "output_mean_accumulate", *s.accumulate(h, v, 0.5, None if null_state else s.u, None if null_state else s.u))
            w(f"{label}: vars {v}", f + "output_mean_get", h, v, s.ptr(mean), t, w.st)
            w(f"{label}: vars {v}", f + "output_mean_reset", h, v, w.st)
            w(f"{label}: vars {v}", f + "output_mean_time", h, v, t)

    w("unknown bits", f + "output_mean_enable", h, 8)
    w("unknown bits", f + "output_mean_enable", h, -1)
    w("nothing", f + "output_mean_enable", h, 0)
    each("unknown bits", (8, 9, 1 << 30))
    each("not enabled", (1, 2, 4, 7))
    for v in (3, 5, 6, 7, 0):
        w(f"two variables or none: {v}", f + "output_mean_get", h, v, s.ptr(mean), t, w.st)
        w(f"two variables or none: {v}", f + "output_mean_time", h, v, t)
    w("solution and sources", f + "output_mean_enable", h, 5)
    each("primitive variables not enabled", (2, 3, 7))
    w("all three, two of them kept", f + "output_mean_enable", h, 7)
    for v in (1, 2, 4):
        w(f"no accumulated time: var {v}", f + "output_mean_get", h, v, s.ptr(mean), t, w.st)
        w(f"no accumulated time: var {v}", f + "output_mean_time", h, v, t, result=lambda: hexbits(np.array(t[:])))
    for v in (1, 2, 3, 4, 7):
        w(f"null state: vars {v}", f + "output_mean_accumulate", *s.accumulate(h, v, 0.5, None, None))
    w("null primitive state", f + "output_mean_accumulate", *s.accumulate(h, 2, 0.5, s.u, None))
    w("null solution state", f + "output_mean_accumulate", *s.accumulate(h, 1, 0.5, None, s.u))
    w("null dts", f + "output_mean_accumulate", *s.accumulate(h, 7, None, s.u, s.u))
    w("one member at 0", f + "output_mean_accumulate", *s.accumulate(h, 7, "one member at 0" if B > 1 else 0.0, s.u, s.u))
    for v in (1, 2, 4):
        w(f"one member at 0: var {v}", f + "output_mean_get", h, v, s.ptr(mean), t, w.st)
    w("all three", f + "output_mean_accumulate", *s.accumulate(h, 7, 0.25, s.u, s.u))
    w("solution and sources", f + "output_mean_accumulate", *s.accumulate(h, 5, 0.5, s.u, None))
    w("nothing", f + "output_mean_accumulate", *s.accumulate(h, 0, 0.5, None, None))
    for v in (1, 2, 4):
        w(f"null d_mean: var {v}", f + "output_mean_get", h, v, None, t, w.st)
        w(f"null time: var {v}", f + "output_mean_time", h, v, None)
        w(f"var {v}", f + "output_mean_get", h, v, s.ptr(mean), t, w.st, result=means())
        w(f"var {v}", f + "output_mean_time", h, v, t, result=lambda: hexbits(np.array(t[:])))
    w("var 1 into an array 8 bytes off a 16-byte boundary", f + "output_mean_get", h, 1, s.ptr(mean) + 8, t, w.st, result=means(1))
    w("var 4 without the time", f + "output_mean_get", h, 4, s.ptr(mean), None, w.st, result=means())
    w("solution", f + "output_mean_reset", h, 1, w.st)
    w("after the reset", f + "output_mean_time", h, 1, t, result=lambda: hexbits(np.array(t[:])))
    w("after the reset", f + "output_mean_get", h, 1, s.ptr(mean), t, w.st)
    w("the others keep theirs", f + "output_mean_get", h, 2, s.ptr(mean), t, w.st, result=means())
    w("solution again", f + "output_mean_accumulate", *s.accumulate(h, 1, 0.125, s.u, None))
    w("solution again", f + "output_mean_get", h, 1, s.ptr(mean), t, w.st, result=means())
    w("all", f + "output_mean_reset", h, 7, w.st)
    w("nothing", f + "output_mean_reset", h, 0, w.st)


def walk_series(w, s, h):
    no, W, B = s.no, s.W, s.B
    sites = np.array([0, no - 1, 7, 7, 20], dtype=np.int32)
    sp = sites.ctypes.data_as(IP)
    e, n, cap = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    times, values = np.full(4 * B, -1.0), np.full(4 * B * sites.size * W, -1.0)
    tp, vp = times.ctypes.data_as(DP), values.ctypes.data_as(DP)

    def call(label, what, *args, result=None):
        name, a = s.series(what, h, *args)
        return w(label, name, *a, result=result)

    def info():
        return [e.value, n.value, cap.value]

    def read(count):
        return lambda: {"times": hexbits(times[: count * B]), "values": hexbits(values[: count * B * sites.size * W])}

    def each(label):
        call(label, "record", 1.0, s.u)
        call(label, "info", C.byref(e), C.byref(n), C.byref(cap))
        call(label, "read", 0, 0, tp, vp)
        call(label, "clear")

    each("not enabled")
    call("negative count", "enable", -1, sp, 2)
    call("negative capacity", "enable", sites.size, sp, -2)
    call("null sites", "enable", sites.size, None, 2)
    for bad in (-1, no, no + 100):
        ids = sites.copy()
        ids[3] = bad
        call(f"site {bad}", "enable", ids.size, ids.ctypes.data_as(IP), 2)
    each("still not enabled")
    call("five sites, two records", "enable", sites.size, sp, 2)
    call("enabled twice", "enable", sites.size, sp, 2)
    call("enabled twice, bad arguments", "enable", -1, None, -1)
    call("empty", "info", C.byref(e), C.byref(n), C.byref(cap), result=info)
    call("no pointers", "info", None, None, None)
    call("empty log", "read", 0, 1, tp, vp)
    call("empty log, nothing asked", "read", 0, 0, None, None)
    call("null u", "record", 1.0, None)
    if B > 1:
        call("null times", "record", None, s.u)
    call("first", "record", 1.5, s.u)
    call("second", "record", 2.75, s.u)
    call("log full", "record", 3.0, s.u)
    call("full", "info", C.byref(e), C.byref(n), C.byref(cap), result=info)
    for first, count in ((1, 2), (-1, 1), (0, -1), (2, 1), (0, 3), (2147483647, 2147483647)):
        call(f"[{first}, {first} + {count}) outside the log", "read", first, count, tp, vp)
    call("null times", "read", 0, 2, None, vp)
    call("null values", "read", 0, 2, tp, None)
    call("both", "read", 0, 2, tp, vp, result=read(2))
    call("the second", "read", 1, 1, tp, vp, result=read(1))
    call("none at the end", "read", 2, 0, None, None)
    call("", "clear")
    call("cleared", "info", C.byref(e), C.byref(n), C.byref(cap), result=info)
    call("cleared", "read", 0, 1, tp, vp)
    call("after the clear", "record", 4.0, s.u)
    call("after the clear", "read", 0, 1, tp, vp, result=read(1))


def walk_swe_only(w, s, h):
    """what the SWE series has beyond the other two: the kind argument, the boundary-flux log and the device log"""
    e, n, cap, t = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_double(-1.0)
    times, values = np.full(2, -1.0), np.full(2 * 64 * 3, -1.0)
    tp, vp = times.ctypes.data_as(DP), values.ctypes.data_as(DP)
    log = C.c_void_p()
    for kind in (0, 3, -1):
        w(f"kind {kind}", "rdyhip_series_record", h, kind, C.c_double(1.0), s.ptr(s.u), w.st)
        w(f"kind {kind}", "rdyhip_series_info", h, kind, C.byref(e), C.byref(n), C.byref(cap), C.byref(t))
        w(f"kind {kind}", "rdyhip_series_read", h, kind, 0, 1, tp, vp, w.st)
        w(f"kind {kind}", "rdyhip_series_device_log", h, kind, C.byref(log))
        w(f"kind {kind}", "rdyhip_series_clear", h, kind)
    for kind in (1, 2):
        w(f"kind {kind} null d_log", "rdyhip_series_device_log", h, kind, None)
    w("not enabled", "rdyhip_series_record", h, 2, C.c_double(1.0), None, w.st)
    w("not enabled", "rdyhip_series_boundary_fluxes_add_time", h, C.c_double(1.0))
    w("not enabled", "rdyhip_series_boundary_edges", h, C.byref(e), None, None)
    w("negative capacity", "rdyhip_series_boundary_fluxes_enable", h, 0, None, -1)
    w("all boundaries, one record", "rdyhip_series_boundary_fluxes_enable", h, 0, None, 1)
    w("enabled twice", "rdyhip_series_boundary_fluxes_enable", h, 0, None, 1)
    w("", "rdyhip_series_boundary_fluxes_add_time", h, C.c_double(0.5))
    w("first", "rdyhip_series_record", h, 2, C.c_double(1.0), None, w.st)
    w("log full", "rdyhip_series_record", h, 2, C.c_double(2.0), None, w.st)
    w("", "rdyhip_series_info", h, 2, C.byref(e), C.byref(n), C.byref(cap), C.byref(t), result=lambda: [e.value, n.value, cap.value, t.value])
    rows = e.value if 0 <= e.value <= 64 else 0
    w("outside the log", "rdyhip_series_read", h, 2, 1, 1, tp, vp, w.st)
    w("null values", "rdyhip_series_read", h, 2, 0, 1, tp, None, w.st)
    w("the record", "rdyhip_series_read", h, 2, 0, 1, tp, vp, w.st, result=lambda: {"times": hexbits(times[:1]), "values": hexbits(values[: rows * 3])})
    w("", "rdyhip_series_clear", h, 2)


def walk_stats(w, s, h):
    out = w.torch.zeros((3, 3, s.no), dtype=w.torch.float64, device="cuda")
    for comps in (0, 8, -1):
        w(f"mask {comps}", "rdyhip_ens_stats", h, comps, s.ptr(s.u), s.ptr(out), w.st)
    w("null u", "rdyhip_ens_stats", h, 7, None, s.ptr(out), w.st)
    w("null d_stats", "rdyhip_ens_stats", h, 7, s.ptr(s.u), None, w.st)
    w("mask 5", "rdyhip_ens_stats", h, 5, s.ptr(s.u), s.ptr(out), w.st, result=lambda: hexbits(out.cpu().numpy()[:, :2]))


def walk_state(w, s, h):
    walk_readout(w, s, h)
    walk_sums(w, s, h)
    walk_means(w, s, h)
    walk_series(w, s, h)
    if isinstance(s, Ens):
        walk_stats(w, s, h)
    elif not isinstance(s, Tracer):
        walk_swe_only(w, s, h)


def run_script(numbering):
    """(the list of records, their labels) of the whole script on one numbering"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mesh = make_mesh(numbering)
    w = Walk()
    w("what rdyhip_last_error() holds from here on until a call fails", "rdyhip_state_read_wait", None)

    def operator():
        op = Operator.create(RDyFlowConfig(), mesh)
        assert op.layout_info()["owned_is_prefix"] == (1 if numbering == "natural" else 0)
        return op

    ops = [operator() for _ in range(3)]
    rng = np.random.default_rng(2036)
    swe = Swe(w, ops[0], rng)
    f = torch.empty((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    ops[0].rhs_function(1e-3, swe.u, f)          # the primitive variables of the means: those of this evaluation, formed on demand
    ops[1].enable_tracers(2)
    ops[2].enable_ensemble(3)
    tracer, ens = Tracer(w, ops[1], rng), Ens(w, ops[2], rng)
    for s in (swe, tracer, ens):
        walk_state(w, s, None)                   # null operator
    for s in (tracer, ens):
        walk_state(w, s, ops[0]._h)              # the feature is not enabled
    for s in (swe, tracer, ens):
        walk_state(w, s, s.h)
    torch.cuda.synchronize()
    for op in ops:
        op.destroy()
    return w.log, w.labels


def dump_golden(golden):
    """The fixture's text.  Most refusals repeat their message and the second numbering answers most calls as the first does, so:
    every entry point and every distinct message once, one per line; the first numbering's records as [entry point, return code,
    message(, result)] by index; of the others the records that differ, by position."""
    first, *rest = NUMBERINGS
    calls = sorted({r["call"] for log in golden.values() for r in log})
    errors = sorted({r["error"] for log in golden.values() for r in log})
    ci, ei = {c: i for i, c in enumerate(calls)}, {e: i for i, e in enumerate(errors)}
    js = lambda v: json.dumps(v, separators=(",", ":"))
    row = lambda r: js([ci[r["call"]], r["rc"], ei[r["error"]]] + ([r["result"]] if "result" in r else []))
    lines = lambda items: ",\n".join(items)
    packed = lambda rows: lines(",".join(rows[i:i + 12]) for i in range(0, len(rows), 12))
    parts = [f'"calls":[\n{lines(js(c) for c in calls)}\n]', f'"errors":[\n{lines(js(e) for e in errors)}\n]',
             f'"{first}":[\n{packed([row(r) for r in golden[first]])}\n]']
    for k in rest:
        assert len(golden[k]) == len(golden[first])
        diff = [f'"{i}":{row(r)}' for i, (r, r0) in enumerate(zip(golden[k], golden[first])) if r != r0]
        parts.append(f'"{k}":{{\n{lines(diff)}\n}}')
    return "{\n" + ",\n".join(parts) + "\n}\n"


def load_golden(path=GOLDEN):
    """{numbering: the list of records} of a fixture written by dump_golden"""
    with open(path) as fh:
        g = json.load(fh)
    rec = lambda r: dict({"call": g["calls"][r[0]], "rc": r[1], "error": g["errors"][r[2]]}, **({"result": r[3]} if len(r) > 3 else {}))
    first, *rest = NUMBERINGS
    out = {first: [rec(r) for r in g[first]]}
    for k in rest:
        out[k] = [rec(g[k][str(i)]) if str(i) in g[k] else r for i, r in enumerate(out[first])]
    return out


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.mark.parametrize("numbering", NUMBERINGS)
def test_every_call_of_the_script_answers_as_the_parent_did(numbering, golden):
    (got, labels), want = run_script(numbering), golden[numbering]
    assert [r["call"] for r in got] == [r["call"] for r in want]
    for g, label, r in zip(got, labels, want):
        assert g == r, (label, g, r)
