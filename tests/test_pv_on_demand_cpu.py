"""The two calls that go with primitive variables on demand (rdyhip_field_release, rdyhip_primitive_variables_stored): exported,
bound, and their argument checks answer before any HIP call -- no device is needed.  What they do to an operator is in
tests/test_gpu_pv_on_demand.py."""
import ctypes as C
import os

from rdycore_amd import _lib

ERR_USER = 83   # PETSC_ERR_USER
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "rdyhip.h")).read()
    for name in ("rdyhip_field_release", "rdyhip_primitive_variables_stored"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
        assert f"int {name}(" in header, name


def test_argument_errors_without_a_device():
    lib = _lib.load()
    out = C.c_int32(-5)
    assert lib.rdyhip_primitive_variables_stored(None, C.byref(out)) == ERR_USER
    assert b"null" in lib.rdyhip_last_error()
    assert out.value == -5
    assert lib.rdyhip_primitive_variables_stored(None, None) == ERR_USER
    assert b"null" in lib.rdyhip_last_error()
    assert lib.rdyhip_field_release(None, 0) == ERR_USER
    assert b"null" in lib.rdyhip_last_error()


def test_release_refuses_every_field_but_the_primitive_variables():
    lib = _lib.load()
    for field in (1, 2, 3, 4, 5, -1):        # external sources, Manning n, flux divergence, gradients, two unknown ids
        assert lib.rdyhip_field_release(None, field) == ERR_USER
        msg = lib.rdyhip_last_error()
        assert b"only the primitive variables" in msg and str(field).encode() in msg, msg
