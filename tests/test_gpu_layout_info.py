"""GPU: what rdyhip_create keeps of the host-side layout pass, and the device buffers that free and regrow themselves.

Three meshes of test_layout_tables_cpu (one tile of triangles; ghosts numbered between the owned cells; quads, second order):
the operator's layout numbers are those of rdyhip_probe_layout in every field but the two only a device gives
(device_bytes, persistent_grid), and device_bytes is the figure recorded in tests/golden/layout_tables.json -- the sum over
the same buffers as before the buffers owned their memory (bench.py compares layout byte counts against stored profiles).
On the one-tile operator the setters' staging buffers are made to grow (8 values, then 48), through the blocking and the
stream-ordered forms, and what was written is read back exactly; the operator is destroyed and created once more at the end.
The probe reports the tiled kernels' layout, so the operators are created with them whatever RDYHIP_KERNEL says.  No assertion
on free device memory: the card is shared."""
import ctypes as C
import json

import numpy as np
import pytest

from rdycore_amd import _lib
from rdycore_amd.operator import Operator, _DeviceArray, probe_layout

from test_layout_tables_cpu import FIRST, GOLDEN, SECOND, case_mesh

pytestmark = pytest.mark.gpu

CASES = [("tri6x4", "first", FIRST), ("interleaved", "first", FIRST), ("quads64x32", "second", SECOND)]


def _read_field(op, field, shape):
    """a host copy of an input field through rdyhip_field_ptr_const (no side effect on the operator)"""
    import torch
    p, n = C.c_void_p(), C.c_int64()
    _lib.check(_lib.load().rdyhip_field_ptr_const(op._h, int(field), C.byref(p), C.byref(n)))
    assert n.value == int(np.prod(shape))
    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceArray(p.value, (n.value,), op), device="cuda").cpu().numpy().reshape(shape)


def _check_info(op, config, mesh, device_bytes):
    got, want = op.layout_info(), probe_layout(config, mesh)
    for k in want:
        if k not in ("device_bytes", "persistent_grid"):
            assert got[k] == want[k], k
    assert got["persistent_grid"] >= 8
    assert got["device_bytes"] == device_bytes


@pytest.mark.parametrize("name,order,config", CASES, ids=[f"{m}-{o}" for m, o, _ in CASES])
def test_operator_keeps_the_probed_layout_and_setters_regrow_their_staging(monkeypatch, name, order, config):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    monkeypatch.delenv("RDYHIP_KERNEL", raising=False)
    with open(GOLDEN) as fh:
        device_bytes = json.load(fh)["device_bytes"][f"{name}-{order}"]
    mesh = case_mesh(name)
    op = Operator.create(config, mesh)
    _check_info(op, config, mesh, device_bytes)
    if name == "tri6x4":
        no = mesh.num_owned_cells
        assert no == 48
        rng = np.random.default_rng(5)
        for ordered in (False, True):
            ids8, v8 = rng.permutation(no)[:8], rng.uniform(0.01, 0.1, 8)
            before = _read_field(op, 2, (no,)).copy()
            op.set_regional_mannings_n(ids8, v8, ordered=ordered)
            want = before
            want[ids8] = v8
            assert np.array_equal(_read_field(op, 2, (no,)), want)
            ids48, v48 = rng.permutation(no), rng.uniform(0.01, 0.1, no)     # more values and ids than the staging buffers hold
            op.set_regional_mannings_n(ids48, v48, ordered=ordered)
            want = np.empty(no)
            want[ids48] = v48
            assert np.array_equal(_read_field(op, 2, (no,)), want)
            water = rng.uniform(0.0, 1e-3, no)
            op.set_domain_external_source(0, water, ordered=ordered)
            src = _read_field(op, 1, (no, 3))
            assert np.array_equal(src[:, 0], water) and not src[:, 1:].any()
        assert op.layout_info()["device_bytes"] == device_bytes      # the staging buffers were never part of the figure
    op.destroy()
    op = Operator.create(config, mesh)
    _check_info(op, config, mesh, device_bytes)
    op.destroy()
