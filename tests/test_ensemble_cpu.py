"""CPU: ensembles (rdyhip_ensemble_*, csrc/ensemble_kernels.h) as far as they go without a device -- the ten symbols and their
null-operator refusal, the eight instantiations of the kernel in the built library and their registers, and the calls
EnsembleEulerStepper makes around a recording stand-in operator."""
import ctypes as C

import numpy as np
import torch

from rdycore_amd import _lib, build, codeobj
from rdycore_amd.timestep import EnsembleEulerStepper

SYMBOLS = ["rdyhip_ensemble_enable", "rdyhip_ensemble_info", "rdyhip_ensemble_set_mannings", "rdyhip_ensemble_set_external_source",
           "rdyhip_ensemble_set_boundary_values", "rdyhip_ensemble_rhs_function", "rdyhip_ensemble_euler_step",
           "rdyhip_ensemble_get_boundary_fluxes", "rdyhip_ensemble_update_diagnostics", "rdyhip_ensemble_get_diagnostics"]


def test_the_ten_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("rdyhip_ensemble_")) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1], name
    assert lib.rdyhip_version() == 110


def test_every_entry_point_reports_a_null_operator():
    lib = _lib.load()
    n = C.c_int32()
    v = (C.c_double * 8)()
    cs = (_lib.RDyHipCourant * 2)()
    calls = {
        "rdyhip_ensemble_enable": (None, 2),
        "rdyhip_ensemble_info": (None, C.byref(n)),
        "rdyhip_ensemble_set_mannings": (None, 0, 1, None, v),
        "rdyhip_ensemble_set_external_source": (None, 0, 0, 1, None, v),
        "rdyhip_ensemble_set_boundary_values": (None, 0, 0, 1, v),
        "rdyhip_ensemble_rhs_function": (None, v, None, None, None),
        "rdyhip_ensemble_euler_step": (None, v, None, None, None, None),
        "rdyhip_ensemble_get_boundary_fluxes": (None, 0, 0, 1, v),
        "rdyhip_ensemble_update_diagnostics": (None, None),
        "rdyhip_ensemble_get_diagnostics": (None, cs),
    }
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())


def test_every_ensemble_kernel_keeps_its_geometry_in_registers():
    """2 slot counts x 2 source methods x with / without the fused Euler update; a per-thread array that went to scratch, or a
    spilled register, shows in the code object's metadata"""
    res = {k: v for k, v in codeobj.kernel_resources(build.lib_path()).items() if "ensemble_rhs_kernel<" in k}
    forms = {k.split("ensemble_rhs_kernel<")[1].split(">")[0] for k in res}
    assert forms == {f"{s}, {src}, {eu}" for s in (3, 4) for src in (0, 1) for eu in ("false", "true")} and len(res) == 8
    bad = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr_spills"] != 0 or v["sgpr_spills"] != 0}
    assert not bad, bad
    assert max(v["vgpr"] + v["agpr"] for v in res.values()) <= 256          # at least two waves per SIMD
    for k in res:                                                           # the families other tests count are what they were
        assert not any(n in k for n in ("swe_rhs_kernel<", "swe_rhs_tiled_kernel<", "swe_rhs_muscl_fused_kernel<", "tracer_rhs_kernel<"))


class RecordingOp:
    """du/dt = lam_m u per member, with the one call the stepper makes"""

    def __init__(self, lams):
        self.lams = np.asarray(lams, dtype=np.float64)
        self.calls = []

    def ensemble_euler_step(self, dts, u_local, u_out, f_global=None):
        assert u_out is not u_local and f_global is None
        self.calls.append((np.array(dts), u_local, u_out))
        for m, (lam, dt) in enumerate(zip(self.lams, dts)):
            u_out[m, :2] = u_local[m, :2] + dt * lam * u_local[m, :2]     # rows 0, 1 are "owned", row 2 is a ghost


def test_stepper_runs_lockstep_fused_steps_on_a_ping_pong_pair():
    op = RecordingOp([-0.5, 0.25])
    st = EnsembleEulerStepper(op)
    u = torch.ones((2, 3, 3), dtype=torch.float64)
    u[:, 2] = 7.0
    dts = [0.1, 0.2]
    out = st.advance(u, dts, 3)
    assert len(op.calls) == 3 and st.step == 3
    assert all(np.array_equal(c[0], np.array(dts)) for c in op.calls)
    # ping-pong: the output of one step is the input of the next, two arrays in all, and the result is in the one returned
    assert op.calls[0][1] is u and op.calls[1][1] is op.calls[0][2] and op.calls[2][1] is u and op.calls[1][2] is u
    assert out is op.calls[2][2] and out is not u
    want = np.array([(1 + 0.1 * -0.5) ** 3, (1 + 0.2 * 0.25) ** 3])
    assert np.allclose(out[:, :2, :].numpy(), want[:, None, None], rtol=1e-15)
    assert (out[:, 2] == 7.0).all()                                        # ghost rows of the second array start as the first one's
    assert np.allclose(st.times, [0.3, 0.6])
    # an even number of steps ends in the caller's array; the second array is kept
    second = out
    op.calls.clear()
    u2 = torch.ones((2, 3, 3), dtype=torch.float64)
    assert st.advance(u2, dts, 2) is u2 and op.calls[0][2] is second and st.step == 5
    assert st.advance(u2, dts, 0) is u2 and len(op.calls) == 2


def test_stepper_takes_its_own_result_back_after_odd_step_counts():
    """a caller that looks at every step: u = advance(u, dts, 1) again and again, and odd counts mixed with even ones.  No step
    may be asked to run in place, the caller's first array is written by no step after it has been left, and the trajectory is
    that of one long advance."""
    lams, dts = [-0.5, 0.25], [0.1, 0.2]
    op = RecordingOp(lams)
    st = EnsembleEulerStepper(op)
    u0 = torch.ones((2, 3, 3), dtype=torch.float64)
    u0[:, 2] = 7.0
    first = u0.clone()
    u = u0
    seen = []
    for n in (1, 1, 1, 3, 2, 1, 5):
        u = st.advance(u, dts, n)
        seen.append(u)
    total = 14
    assert st.step == total and len(op.calls) == total
    assert all(c[1] is not c[2] for c in op.calls)                          # RecordingOp asserts it too: never in place
    assert all(op.calls[k + 1][1] is op.calls[k][2] for k in range(total - 1))   # every step starts from the previous step's output
    assert all(c[2] is not u0 for c in op.calls) and torch.equal(u0, first)  # u0 was read by the first step and never written
    assert len({id(c[2]) for c in op.calls}) == 2 and all(x is not u0 for x in seen)   # two arrays of the stepper's own
    want = np.array([(1 + dt * lam) ** total for lam, dt in zip(lams, dts)])
    assert np.allclose(u[:, :2, :].numpy(), want[:, None, None], rtol=1e-14) and (u[:, 2] == 7.0).all()
    assert np.allclose(st.times, [total * 0.1, total * 0.2])
    one = EnsembleEulerStepper(RecordingOp(lams)).advance(u0.clone(), dts, total)
    assert torch.equal(one, u)
