"""CPU: the state read-out (rdyhip_state_planes, rdyhip_state_read_*, rdyhip_error_sums; csrc/readout_kernels.h) as far as it
goes without a device -- the symbols and the ctypes table, the argument errors that are reported before any device call, the
constants of operator.py against the header's, and the three kernels in the code object."""
import ctypes as C
import os
import re

import pytest

from rdycore_amd import _lib, build
from rdycore_amd import operator as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rdyhip_state_planes", "rdyhip_state_read_begin", "rdyhip_state_read_ready", "rdyhip_state_read_wait", "rdyhip_state_read_get",
               "rdyhip_state_read_ptr", "rdyhip_error_sums", "rdyhip_error_sums_get"]


def header_defines():
    with open(os.path.join(ROOT, "include", "rdyhip.h")) as fh:
        return {k: int(v) for k, v in re.findall(r"^#define (RDYHIP_[A-Z_0-9]+) (\d+)\s*$", fh.read(), flags=re.M)}


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.rdyhip_version() == 110
    assert C.sizeof(_lib.RDyHipErrorSums) == 80


def test_null_operator_is_a_user_error_before_any_device_call():
    lib = _lib.load()
    n, s = C.c_int32(), _lib.RDyHipErrorSums()
    p = _lib.c_double_p()
    v = (C.c_double * 4)()
    calls = [lambda: lib.rdyhip_state_planes(None, 7, None, None, None),
             lambda: lib.rdyhip_state_read_begin(None, 1, None, None),
             lambda: lib.rdyhip_state_read_ready(None, C.byref(n)),
             lambda: lib.rdyhip_state_read_wait(None),
             lambda: lib.rdyhip_state_read_get(None, 1, 4, v),
             lambda: lib.rdyhip_state_read_ptr(None, 1, C.byref(p)),
             lambda: lib.rdyhip_error_sums(None, None, None, None),
             lambda: lib.rdyhip_error_sums_get(None, C.byref(s))]
    for call in calls:
        assert call() == 83                                      # PETSC_ERR_USER
        assert b"null" in lib.rdyhip_last_error()


def test_component_constants_equal_the_headers():
    d = header_defines()
    assert (O.COMPONENT_H, O.COMPONENT_HU, O.COMPONENT_HV) == (d["RDYHIP_COMPONENT_H"], d["RDYHIP_COMPONENT_HU"], d["RDYHIP_COMPONENT_HV"]) == (1, 2, 4)
    assert d["RDYHIP_ERROR_SUMS_BLOCK"] == 256 and d["RDYHIP_ERROR_SUMS_MAX_WORKGROUPS"] == 1024


def test_readout_kernels_are_in_the_code_object_without_scratch():
    pytest.importorskip("msgpack")
    from rdycore_amd import codeobj
    res = codeobj.kernel_resources(build.lib_path())
    for kernel, lds in (("state_planes_kernel", 0), ("error_partial_kernel", 320), ("error_finalize_kernel", 320)):
        forms = {k: v for k, v in res.items() if f"rdyhip::{kernel}" in k}
        assert len(forms) == 1, (kernel, sorted(forms))
        for k, v in forms.items():
            assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
            assert v["lds"] == lds, (k, v)                       # the folds' [4 waves][10] doubles; the de-interleave needs none
    # the RHS kernels are what they were: 84 tiled / fused instantiations + 4 cell-centric ones
    assert sum("swe_rhs_tiled_kernel<" in k or "swe_rhs_muscl_fused_kernel<" in k for k in res) == 84
    assert sum("swe_rhs_kernel<" in k for k in res) == 4
