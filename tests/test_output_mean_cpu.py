"""CPU: the time-averaged output fields (rdyhip_output_mean_*, csrc/output_kernels.h) as far as they go without a device --
the symbols and their argument errors, the two kernels in the code object, and which calls EulerStepper(means=...) makes
around a stand-in operator that records them."""
import ctypes as C
import types

import pytest
import torch

from rdycore_amd import _lib, build
from rdycore_amd.timestep import EulerStepper


def test_argument_errors_without_a_device():
    lib = _lib.load()
    t = C.c_double()
    calls = [lambda: lib.rdyhip_output_mean_enable(None, 7),
             lambda: lib.rdyhip_output_mean_accumulate(None, 7, 0.1, None, None),
             lambda: lib.rdyhip_output_mean_get(None, 1, None, C.byref(t), None),
             lambda: lib.rdyhip_output_mean_reset(None, 7, None),
             lambda: lib.rdyhip_output_mean_time(None, 1, C.byref(t))]
    for call in calls:
        # PETSC_ERR_USER = 83, reported before any HIP call
        assert call() == 83
        assert b"null" in lib.rdyhip_last_error()


def test_the_bits_of_the_header_and_the_operator_module_agree():
    from rdycore_amd import operator as O
    assert (O.OUTPUT_SOLUTION, O.OUTPUT_PRIMITIVE_VARIABLES, O.OUTPUT_SOURCES) == (1, 2, 4)


def test_accumulate_and_mean_kernels_are_in_the_code_object_without_scratch():
    pytest.importorskip("msgpack")
    from rdycore_amd import codeobj
    res = codeobj.kernel_resources(build.lib_path())
    # the accumulate kernel has one form (a lane per cell), the element-wise mean kernel a 16-byte and an 8-byte one
    for kernel, nforms in (("output_accumulate_kernel", 1), ("output_mean_kernel", 2)):
        forms = {k: v for k, v in res.items() if f"rdyhip::{kernel}" in k}
        assert len(forms) == nforms, (kernel, sorted(forms))
        for k, v in forms.items():
            assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["lds"] == 0, (k, v)
    # the RHS kernels are what they were: 84 tiled / fused instantiations + 4 cell-centric ones
    assert sum("swe_rhs_tiled_kernel<" in k or "swe_rhs_muscl_fused_kernel<" in k for k in res) == 84
    assert sum("swe_rhs_kernel<" in k for k in res) == 4


class RecordingOp:
    """du/dt = lam * u with every call the stepper can make, recorded in order"""

    def __init__(self, n, with_rk4_step=True, lam=-0.2):
        self.mesh = types.SimpleNamespace(num_owned_cells=n)
        self.lam = lam
        self.log = []
        if with_rk4_step:
            self.rk4_step = self._rk4_step

    def rhs_function(self, dt, u_local, f_global):
        self.log.append(("rhs", dt, u_local))
        f_global.copy_(self.lam * u_local[: self.mesh.num_owned_cells])

    def axpy_owned(self, a, f_global, u_local):
        self.log.append(("axpy", a, u_local))
        u_local[: self.mesh.num_owned_cells] += a * f_global

    def euler_step(self, dt, u_local, u_out):
        self.log.append(("euler", dt, u_local, u_out))
        u_out.copy_(u_local * (1.0 + dt * self.lam))

    def _rk4_step(self, dt, u_local, halo=None):
        self.log.append(("rk4", dt, u_local))

    def reset_diagnostics(self):
        pass

    def enable_output_means(self, vars):
        self.log.append(("enable", vars))

    def accumulate_output_means(self, vars, dt, u_local=None):
        self.log.append(("accumulate", vars, dt, u_local))

    def output_mean(self, var):
        self.log.append(("get", var))
        return "mean", 1.5

    def reset_output_means(self, vars):
        self.log.append(("reset", vars))

    def output_mean_time(self, var):
        self.log.append(("time", var))
        return 0.0

    def named(self, *names):
        return [e for e in self.log if e[0] in names]


NEW_CALLS = ("enable", "accumulate", "get", "reset", "time")


@pytest.mark.parametrize("temporal,fused", [("euler", True), ("euler", False), ("rk4", True), ("rk4", False)])
def test_without_means_the_stepper_makes_none_of_the_new_calls(temporal, fused):
    op = RecordingOp(3)
    u = torch.ones((3, 3), dtype=torch.float64)
    st = EulerStepper(op, temporal=temporal, fused=fused)
    assert st.means == 0
    st.advance(u, 0.3, 1.0)
    assert st.step == 4 and op.named(*NEW_CALLS) == []


def _two_intervals(temporal, fused, means=7):
    """0.3 + 0.3 + 0.3 + 0.1, twice: a shortened last step in either interval"""
    op = RecordingOp(3)
    u = torch.ones((3, 3), dtype=torch.float64)
    st = EulerStepper(op, temporal=temporal, fused=fused, means=means)
    assert op.log == [("enable", means)]
    st.advance(u, 0.3, 1.0)
    first = len(op.log)
    st.advance(u, 0.3, 1.0)
    assert st.step == 8
    return op, st, u, op.log[1:first], op.log[first:]


def test_fused_euler_accumulates_the_output_array_after_every_step_with_the_intervals_dt():
    op, st, u, first, second = _two_intervals("euler", True)
    for k, part in enumerate((first, second)):
        acc = [i for i, e in enumerate(part) if e[0] == "accumulate"]
        steps = [i for i, e in enumerate(part) if e[0] == "euler"]
        assert len(steps) == 4 and len(acc) == (5 if k == 0 else 4)           # 1 + steps in the first interval, steps afterwards
        assert all(part[i][1] == 7 and part[i][2] == 0.3 for i in acc)        # the interval's dt, also after the step of 0.1
        assert part[steps[3]][1] < 0.3
        if k == 0:
            assert acc[0] == 0 and part[0][3] is u                            # the initial state, before the first step
            acc = acc[1:]
        # one accumulate right behind each step, on the array that step wrote (the previous state is the operator's business)
        for s, a in zip(steps, acc):
            assert a == s + 1 and part[a][3] is part[s][3] and part[s][3] is not part[s][2]


def test_unfused_euler_accumulates_between_the_rhs_and_the_axpy_and_the_solution_after_it():
    op, st, u, first, second = _two_intervals("euler", False)
    assert first[0][:3] == ("accumulate", 7, 0.3) and first[0][3] is u
    for k, part in enumerate((first[1:], second)):
        assert [e[0] for e in part] == ["rhs", "accumulate", "axpy", "accumulate"] * 4
        for i in range(0, len(part), 4):
            rhs, a1, axpy, a2 = part[i:i + 4]
            assert a1 == ("accumulate", 6, 0.3, None)                         # primitive variables | sources: of the state the RHS saw
            assert a2[:3] == ("accumulate", 1, 0.3) and a2[3] is u            # the solution: after the update
            assert rhs[1] == axpy[1] and (rhs[1] == 0.3 or i == 12)
        assert part[12][1] < 0.3
    assert len(op.named("accumulate")) == 1 + 2 * 8


def test_a_subset_of_the_variables_makes_only_the_calls_it_needs():
    op, st, u, first, second = _two_intervals("euler", False, means=1)
    assert all(e[1] == 1 and e[3] is u for e in op.named("accumulate")) and len(op.named("accumulate")) == 1 + 8
    op, st, u, first, second = _two_intervals("euler", False, means=4)
    assert all(e[1:] == (4, 0.3, None) for e in op.named("accumulate")[1:]) and len(op.named("accumulate")) == 1 + 8


@pytest.mark.parametrize("fused", [True, False])
def test_rk4_accumulates_once_after_the_step(fused):
    op, st, u, first, second = _two_intervals("rk4", fused)
    assert first[0][:3] == ("accumulate", 7, 0.3) and first[0][3] is u
    for part in (first[1:], second):
        acc = [e for e in part if e[0] == "accumulate"]
        assert len(acc) == 4 and all(e[1:3] == (7, 0.3) and e[3] is u for e in acc)
        if fused:
            assert [e[0] for e in part] == ["rk4", "accumulate"] * 4
        else:
            # the loop's last call of a step is the fourth axpy into u; the accumulate follows it
            idx = [i for i, e in enumerate(part) if e[0] == "accumulate"]
            assert all(part[i - 1][0] == "axpy" and part[i - 1][2] is u for i in idx)
            assert len([e for e in part if e[0] == "rhs"]) == 16


def test_output_mean_of_the_stepper_is_get_then_reset():
    op = RecordingOp(3)
    st = EulerStepper(op, means=5)
    op.log.clear()
    assert st.output_mean(4) == ("mean", 1.5)
    assert op.log == [("get", 4), ("reset", 4)]


def test_mean_client_compiles_as_c11(tmp_path):
    import os
    from test_gpu_c_client import compile_client
    assert os.path.exists(compile_client(tmp_path, "rdyhip_mean_client"))
