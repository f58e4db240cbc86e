"""GPU: the state read-out from a plain C host (tests/c_client/rdyhip_read_client.c): fused Euler steps on ex2b, and after every
interval the three owned-cell planes through rdyhip_state_read_begin / the next interval's steps / _wait / _get / _ptr --
against the Python stepper's state columns, bit for bit, and the final rdyhip_error_sums against Operator.error_sums."""
import os
import struct
import subprocess

import numpy as np
import pytest

from rdycore_amd import build
from rdycore_amd import cases as CS
from rdycore_amd.timestep import EulerStepper

from test_gpu_c_client import compile_client, write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_client_compiles_as_c11(tmp_path):
    """gcc -std=c11 -Wall -Werror against include/rdyhip.h, linked with librdyhip.so (no GPU needed for that)"""
    assert os.path.exists(compile_client(tmp_path, "rdyhip_read_client"))


@pytest.mark.gpu
def test_c_host_reads_the_planes_of_every_interval_on_ex2b(tmp_path):
    import torch
    build.build_native()
    case = CS.ex2b_case(os.path.join(ROOT, "tests", "golden", "planar_dam_10x5.msh"))
    mesh = case.mesh
    no = mesh.num_owned_cells
    nint, steps = 5, 24
    interval = steps * case.dt
    path, out_path = str(tmp_path / "ex2b.bin"), str(tmp_path / "out.bin")
    write_case(path, case, True, np.zeros((no, 3)), np.zeros((no, 3)), np.zeros((no, 3)), 0.0)
    exe = compile_client(tmp_path, "rdyhip_read_client")
    env = dict(os.environ)
    env.pop("RDYHIP_LIB", None)
    run = subprocess.run([exe, path, out_path, str(nint), repr(interval), repr(case.dt)], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = open(out_path, "rb").read()
    assert struct.unpack("2i", raw[:8]) == (nint, no)
    planes = np.frombuffer(raw[8:8 + 8 * 3 * no * nint], dtype=np.float64).reshape(nint, 3, no)
    sums_c = np.frombuffer(raw[8 + 8 * 3 * no * nint:], dtype=np.float64)
    assert sums_c.size == 10

    # the same intervals through the Python stepper
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    st = EulerStepper(op)
    own = np.asarray(mesh.cell_owned_to_local)
    moved = 0.0
    for iv in range(nint):
        st.advance(u, case.dt, interval)
        ref = u.cpu().numpy()[own]
        for c in range(3):
            assert np.array_equal(planes[iv, c].view(np.int64), np.ascontiguousarray(ref[:, c]).view(np.int64)), (iv, c)
        moved = max(moved, float(np.abs(ref[:, 0] - case.u_local[own, 0]).max()))
    assert st.step >= nint * steps and moved > 1e-3               # the dam has started to break: the intervals differ
    assert not np.array_equal(planes[0], planes[-1])
    s = op.error_sums(u)
    got = np.concatenate([s["l1"], s["l2_squared"], s["linf"], [s["area"]]])
    assert np.array_equal(sums_c.view(np.int64), got.view(np.int64)), (sums_c, got)
    assert sums_c[9] > 0.0 and sums_c[0] > 0.0
    op.destroy()
