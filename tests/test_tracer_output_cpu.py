"""Tracer output (rdyhip_tracer_state_* / _error_sums / _output_mean_* / _series_*, csrc/tracer_output_kernels.h) without a
device: the symbols and their signatures, the refusals that need no operator, and the resources of the built kernels."""
import ctypes as C
import os
import re

from rdycore_amd import _lib, build, codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["state_planes", "state_read_begin", "state_read_ready", "state_read_wait", "state_read_get", "state_read_ptr", "error_sums",
         "error_sums_get", "output_mean_enable", "output_mean_accumulate", "output_mean_get", "output_mean_reset", "output_mean_time",
         "series_enable", "series_record", "series_info", "series_read", "series_clear"]
CTYPE = {"RDyHipOperator": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double}


def _declarations():
    """name -> list of argument types as the header spells them, comments stripped"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdyhip.h")).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint (rdyhip_tracer_(?:state|error|output|series)[a-z_]*)\s*\(([^)]*)\)\s*;", src):
        out[name] = [" ".join(a.split()) for a in args.split(",")]
    return out


def test_every_entry_point_is_declared_exported_and_bound():
    decl = _declarations()
    assert sorted(decl) == sorted("rdyhip_tracer_" + n for n in NAMES)
    lib = _lib.load()
    for name in decl:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name


def test_argtypes_match_the_header():
    for name, args in _declarations().items():
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args), name
        for text, ct in zip(args, argtypes):
            base = text.replace("const ", "").rsplit(" ", 1)[0].strip()          # "double *", "int32_t", "RDyHipTracerErrorSums *"
            if "*" in text:
                # a pointer in the header is a pointer (or void *) in the table, never a by-value scalar
                assert ct is C.c_void_p or hasattr(ct, "_type_") and not isinstance(ct._type_, str), (name, text, ct)
                if ct is not C.c_void_p and base.startswith("double *") and "**" not in text:
                    assert ct._type_ is C.c_double, (name, text)
                if ct is not C.c_void_p and base.startswith("int32_t"):
                    assert ct._type_ is C.c_int32, (name, text)
            else:
                assert ct is CTYPE[base], (name, text, ct)
    assert C.sizeof(_lib.RDyHipTracerErrorSums) == 8 * 31


def test_every_entry_point_reports_a_null_operator_first():
    lib = _lib.load()
    i, j, k, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    p = _lib.c_double_p()
    v = (C.c_double * 8)()
    ids = (C.c_int32 * 2)()
    s = _lib.RDyHipTracerErrorSums()
    calls = {
        "state_planes": (None, 1, 0, None, None, None),
        "state_read_begin": (None, 0x7FFFFFFF, 9, None, None),          # every other argument is wrong as well: the operator comes first
        "state_read_ready": (None, C.byref(i)),
        "state_read_wait": (None,),
        "state_read_get": (None, 1, 3, v),
        "state_read_ptr": (None, 1, C.byref(p)),
        "error_sums": (None, None, None, None),
        "error_sums_get": (None, C.byref(s)),
        "output_mean_enable": (None, 64),
        "output_mean_accumulate": (None, 7, 0.1, None, None, None),
        "output_mean_get": (None, 1, None, C.byref(d), None),
        "output_mean_reset": (None, 7, None),
        "output_mean_time": (None, 1, C.byref(d)),
        "series_enable": (None, -1, ids, -1),
        "series_record": (None, 0.0, None, None),
        "series_info": (None, C.byref(i), C.byref(j), C.byref(k)),
        "series_read": (None, 0, 1, v, v, None),
        "series_clear": (None,),
    }
    assert sorted(calls) == sorted(NAMES)
    for name, args in calls.items():
        assert getattr(lib, "rdyhip_tracer_" + name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())


def test_every_kernel_keeps_rows_and_sums_in_registers():
    """7 tracer counts x (planes in two forms, partial sums, final sums, accumulate, observe); a per-thread array that went to
    scratch, or a spilled register, shows in the code object's metadata"""
    res = codeobj.kernel_resources(build.lib_path())
    families = {"tracer_planes_kernel<": 14, "tracer_error_partial_kernel<": 7, "tracer_error_finalize_kernel<": 7,
                "tracer_output_accumulate_kernel<": 7, "tracer_series_observe_kernel<": 7}
    for fam, count in families.items():
        mine = {k: v for k, v in res.items() if fam in k}
        forms = {k.split(fam)[1].split(">")[0].split(",")[0] for k in mine}
        assert len(mine) == count and forms == {str(nt) for nt in range(1, 8)}, (fam, sorted(mine))
        bad = {k: v for k, v in mine.items() if v["scratch"] != 0 or v["vgpr_spills"] != 0 or v["sgpr_spills"] != 0}
        assert not bad, bad
        assert max(v["vgpr"] + v["agpr"] for v in mine.values()) <= 256, fam      # a workgroup of 256 lanes still fits a CU
    # the sums of the widest row: 31 doubles per lane in registers, the fold through LDS only
    sums = [v for k, v in res.items() if "tracer_error_partial_kernel<7>" in k]
    assert len(sums) == 1 and sums[0]["lds"] == 4 * 31 * 8
