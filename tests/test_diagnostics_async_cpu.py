"""CPU: the non-blocking Courant read-back (rdyhip_diagnostics_begin / _ready / _wait, csrc/diagnostics_calls.h) as far as it goes
without a device -- the three symbols and their null-operator refusal, the C host that uses them, and the calls
EulerStepper(pipelined=True) makes around a recording stand-in operator with a scripted list of Courant numbers."""
import ctypes as C
import os
import types

import torch

from rdycore_amd import _lib
from rdycore_amd.operator import CourantNumberDiagnostics
from rdycore_amd.timestep import AdaptiveTime, EulerStepper

SYMBOLS = ["rdyhip_diagnostics_begin", "rdyhip_diagnostics_ready", "rdyhip_diagnostics_wait"]


def test_the_three_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("rdyhip_diagnostics_")) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1], name
    assert lib.rdyhip_version() == 110


def test_every_entry_point_reports_a_null_operator():
    lib = _lib.load()
    r = C.c_int32()
    calls = {"rdyhip_diagnostics_begin": (None, 0, None), "rdyhip_diagnostics_ready": (None, 0, C.byref(r)), "rdyhip_diagnostics_wait": (None, 0)}
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())


def test_the_pipeline_client_compiles_as_c11(tmp_path):
    from test_gpu_c_client import compile_client
    assert os.path.exists(compile_client(tmp_path, "rdyhip_pipeline_client"))


class RecordingOp:
    """The calls the stepper makes, by name, and a scripted Courant number per interval: the blocking update delivers the
    current interval's number, begin captures it and wait delivers what the last begin captured."""

    def __init__(self, script):
        self.mesh = types.SimpleNamespace(num_owned_cells=2)
        self.script = list(script)
        self.interval = 0
        self.calls = []
        self.captured = None
        self.current = CourantNumberDiagnostics(0.0, -1, -1)

    def reset_diagnostics(self):
        self.calls.append("reset_diagnostics")

    def euler_step(self, dt, u_local, u_out, f_global=None):
        self.calls.append("euler_step")
        u_out.copy_(u_local)

    def _next(self):
        c = self.script[self.interval]
        self.interval += 1
        return CourantNumberDiagnostics(c, 7, 3)

    def update_diagnostics(self):
        self.calls.append("update_diagnostics")
        self.current = self._next()

    def diagnostics_begin(self):
        self.calls.append("diagnostics_begin")
        self.captured = self._next()

    def diagnostics_wait(self):
        self.calls.append("diagnostics_wait")
        assert self.captured is not None, "wait with no read in flight"
        self.current, self.captured = self.captured, None

    def get_diagnostics(self):
        return self.current


class RecordingForcing:
    def __init__(self, op):
        self.op = op

    def apply(self, time):
        self.op.calls.append("forcing.apply")


# target 0.5, max increase 2, intervals of 0.5 s from dt = 0.1: 0.8 -> a decrease (x 0.625); 0.1 -> the capped increase (x 2, not
# x 5); 0.4 -> an increase below the cap (x 1.25); 0.05 and 0.0 -> x 2 each, the second one past the interval: clamped to 0.5
SCRIPT = [0.8, 0.1, 0.4, 0.05, 0.0, 0.3]
EXPECTED_DT = [0.1, 0.1 * (0.5 / 0.8), 0.1 * (0.5 / 0.8) * 2.0, 0.1 * (0.5 / 0.8) * 2.0 * (0.5 / 0.4), 0.1 * (0.5 / 0.8) * 2.0 * (0.5 / 0.4) * 2.0, 0.5]


def run(pipelined, adaptive=True, intervals=6, with_forcing=True):
    op = RecordingOp(SCRIPT)
    st = EulerStepper(op, adaptive=AdaptiveTime(0.5, 2.0) if adaptive else None, forcing=RecordingForcing(op) if with_forcing else None,
                      pipelined=pipelined)
    u = torch.zeros((3, 3), dtype=torch.float64)
    dt, dts, per_interval = 0.1, [], []
    for _ in range(intervals):
        n0 = len(op.calls)
        dt = st.advance(u, dt, 0.5)
        dts.append(dt)
        per_interval.append(op.calls[n0:])
    return op, st, dts, per_interval


def test_pipelined_call_order():
    op, st, dts, per = run(True)
    for k, calls in enumerate(per):
        steps = [c for c in calls if c == "euler_step"]
        head = ["forcing.apply"] + (["diagnostics_wait"] if k > 0 else []) + ["reset_diagnostics"]
        assert calls == head + steps + ["diagnostics_begin"] and len(steps) >= 1, (k, calls)
    assert "update_diagnostics" not in op.calls


def test_default_keeps_the_blocking_sequence():
    op, st, dts, per = run(False)
    for calls in per:
        steps = [c for c in calls if c == "euler_step"]
        assert calls == ["forcing.apply", "reset_diagnostics"] + steps + ["update_diagnostics"], calls
    assert not any(c.startswith("diagnostics_") for c in op.calls)


def test_pipelined_dt_sequence_is_the_blocking_one():
    _, _, blocking, per_b = run(False)
    _, _, pipelined, per_p = run(True)
    assert pipelined == blocking                       # the same floats, not approximately
    assert blocking == EXPECTED_DT
    assert blocking[1] < blocking[0]                                    # a decrease
    assert blocking[2] == 2.0 * blocking[1] and 0.5 / SCRIPT[1] > 2.0   # an increase, capped
    assert blocking[4] * 2.0 > 0.5 and blocking[5] == 0.5               # dt > interval: clamped
    assert [c.count("euler_step") for c in per_p] == [c.count("euler_step") for c in per_b]


def test_reading_max_courant_collects():
    op, st, _, _ = run(True, intervals=2)
    assert op.calls[-1] == "diagnostics_begin"
    assert st.max_courant == SCRIPT[1]
    assert op.calls[-1] == "diagnostics_wait"
    n = len(op.calls)
    assert st.courant == CourantNumberDiagnostics(SCRIPT[1], 7, 3) and st.max_courant == SCRIPT[1] and len(op.calls) == n   # once
    # the next advance has nothing left to wait for
    before = len(op.calls)
    st.advance(torch.zeros((3, 3), dtype=torch.float64), 0.1, 0.5)
    assert "diagnostics_wait" not in op.calls[before:]


def test_finish_collects_at_the_end_of_a_run():
    op, st, _, _ = run(True, intervals=3)
    st.finish()
    assert op.calls[-1] == "diagnostics_wait" and op.captured is None
    n = len(op.calls)
    st.finish()
    assert len(op.calls) == n and st.max_courant == SCRIPT[2]
    blocking = run(False, intervals=3)[1]
    blocking.finish()                                   # nothing to collect
    assert blocking.max_courant == SCRIPT[2]


def test_without_adaptive_no_diagnostics_call_is_made():
    for pipelined in (True, False):
        op, st, dts, _ = run(pipelined, adaptive=False, intervals=3)
        assert not any(c in ("update_diagnostics", "diagnostics_begin", "diagnostics_wait") for c in op.calls)
        assert dts == [0.1, 0.1, 0.1] and st.max_courant is None
        st.finish()
        assert not any(c in ("update_diagnostics", "diagnostics_begin", "diagnostics_wait") for c in op.calls)
