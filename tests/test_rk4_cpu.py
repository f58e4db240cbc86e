"""CPU: the classical Runge-Kutta step behind the C ABI (rdyhip_rk4_step, csrc/rk_kernels.h) as far as it goes without a
device -- the symbol and its argument errors, the two update kernels in the code object, and which path
EulerStepper(temporal="rk4") takes around a stand-in operator."""
import ctypes as C
import types

import pytest
import torch

from rdycore_amd import _lib, build
from rdycore_amd.timestep import EulerStepper


def test_argument_errors_without_a_device():
    lib = _lib.load()
    # PETSC_ERR_USER = 83, reported before any HIP call
    assert lib.rdyhip_rk4_step(None, None, 0.1, None, None) == 83
    assert b"null operator" in lib.rdyhip_last_error()


def test_stage_and_combine_kernels_are_in_the_code_object_without_scratch():
    pytest.importorskip("msgpack")
    from rdycore_amd import codeobj
    res = codeobj.kernel_resources(build.lib_path())
    for kernel in ("rk4_stage_kernel", "rk4_combine_kernel"):
        forms = {k: v for k, v in res.items() if f"rdyhip::{kernel}<" in k}
        assert len(forms) == 2, (kernel, sorted(forms))                  # the 16-byte and the 8-byte form
        for k, v in forms.items():
            assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["lds"] == 0, (k, v)
            assert "swe_rhs" not in k
    # the RHS kernels are what they were: 84 tiled / fused instantiations + 4 cell-centric ones
    assert sum("swe_rhs_tiled_kernel<" in k or "swe_rhs_muscl_fused_kernel<" in k for k in res) == 84
    assert sum("swe_rhs_kernel<" in k for k in res) == 4


class LoopOp:
    """du/dt = lam * u with the calls the stepper's own Runge-Kutta loop makes"""

    def __init__(self, n, lam=-0.2):
        self.mesh = types.SimpleNamespace(num_owned_cells=n)
        self.lam = lam
        self.rhs_calls = 0
        self.axpy_calls = 0

    def rhs_function(self, dt, u_local, f_global):
        self.rhs_calls += 1
        f_global.copy_(self.lam * u_local[: self.mesh.num_owned_cells])

    def axpy_owned(self, a, f_global, u_local):
        self.axpy_calls += 1
        u_local[: self.mesh.num_owned_cells] += a * f_global

    def reset_diagnostics(self):
        pass


class StepOp(LoopOp):
    """the same with the one-call step"""

    def __init__(self, n):
        super().__init__(n)
        self.steps = []

    def rk4_step(self, dt, u_local, halo=None):
        self.steps.append((dt, u_local, halo))


def test_stepper_makes_one_call_per_step_where_the_operator_has_the_step():
    op = StepOp(3)
    st = EulerStepper(op, temporal="rk4")
    u = torch.ones((3, 3), dtype=torch.float64)
    dt = st.advance(u, 0.3, 1.0)                       # 0.3 + 0.3 + 0.3 + 0.1 (TS_EXACTFINALTIME_MATCHSTEP)
    assert dt == 0.3 and st.step == 4 and abs(st.time - 1.0) < 1e-14
    assert len(op.steps) == 4 and op.rhs_calls == 0 and op.axpy_calls == 0
    assert [s[0] for s in op.steps[:3]] == [0.3, 0.3, 0.3] and abs(op.steps[3][0] - 0.1) < 1e-14 and op.steps[3][0] < 0.3
    assert all(s[1] is u and s[2] is None for s in op.steps)
    # a halo of one rank has nothing to exchange; one with the exchange behind the C ABI is handed on
    one = types.SimpleNamespace(world=1, _halo=None)
    op = StepOp(3)
    EulerStepper(op, halo=one, temporal="rk4").advance(u, 0.5, 0.5)
    assert len(op.steps) == 1 and op.steps[0][2] is None
    chalo = types.SimpleNamespace(world=3, _halo=object(), invalidate=lambda: None)
    op = StepOp(3)
    EulerStepper(op, halo=chalo, temporal="rk4").advance(u, 0.5, 0.5)
    assert len(op.steps) == 1 and op.steps[0][2] is chalo


def test_stepper_keeps_its_loop_without_the_step_or_when_asked_to():
    u = torch.ones((3, 3), dtype=torch.float64)
    op = LoopOp(3)
    EulerStepper(op, temporal="rk4").advance(u, 0.25, 0.5)               # fused by default, but the operator has no rk4_step
    assert op.rhs_calls == 8 and op.axpy_calls == 14
    op = StepOp(3)
    EulerStepper(op, fused=False, temporal="rk4").advance(u, 0.25, 0.5)
    assert op.steps == [] and op.rhs_calls == 8 and op.axpy_calls == 14
    # a halo whose ghost update is driven from Python (transport="torch") keeps the loop as well
    calls = []
    phalo = types.SimpleNamespace(world=3, _halo=None, rhs_overlapped=lambda o, dt, u_, f: (calls.append(dt), f.zero_()))
    op = StepOp(3)
    EulerStepper(op, halo=phalo, temporal="rk4").advance(u, 0.5, 0.5)
    assert op.steps == [] and len(calls) == 4
