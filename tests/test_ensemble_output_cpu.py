"""Ensemble output (rdyhip_ens_state_* / _error_sums / _output_mean_* / _series_* / _stats, csrc/ens_output_kernels.h) without a
device: the symbols and their signatures, the refusals that need no operator, the resources of the built kernels, and the rule of
the member statistics restated in numpy (test_gpu_ensemble_output.py imports it)."""
import ctypes as C
import os
import re

import numpy as np

from rdycore_amd import _lib, build, codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["state_planes", "state_read_begin", "state_read_ready", "state_read_wait", "state_read_get", "state_read_ptr", "error_sums",
         "error_sums_get", "output_mean_enable", "output_mean_accumulate", "output_mean_get", "output_mean_reset", "output_mean_time",
         "series_enable", "series_record", "series_info", "series_read", "series_clear", "stats"]
CTYPE = {"RDyHipOperator": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double}


def _declarations():
    """name -> list of argument types as the header spells them, comments stripped"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdyhip.h")).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint (rdyhip_ens_(?:state|error|output|series|stats)[a-z_]*)\s*\(([^)]*)\)\s*;", src):
        out[name] = [" ".join(a.split()) for a in args.split(",")]
    return out


def ensemble_stats_rule(x):
    """x [B, n] -> (mean, min, max) [3, n] by the rule of rdyhip_ens_stats, in an explicit member loop: the mean adds the members in
    order and multiplies by 1.0 / B once; minimum and maximum start from member 0 and take a later member only where it compares
    strictly below / above the running value -- so of values that compare equal (+0.0 and -0.0 too) the earlier member's bits stay,
    a NaN in a later member is passed over and a NaN in member 0 stays"""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    s, lo, hi = x[0].copy(), x[0].copy(), x[0].copy()
    with np.errstate(invalid="ignore"):
        for m in range(1, B):
            s = s + x[m]
            lo = np.where(x[m] < lo, x[m], lo)
            hi = np.where(x[m] > hi, x[m], hi)
        return np.stack([s * (1.0 / B), lo, hi])


def planted_rows(B):
    """[B, 8] hand-made columns for B >= 3 members: +0.0 before -0.0, -0.0 before +0.0, a tie of the extremes between members, a NaN
    with a payload in member 0, one in a later member, a denormal, and two ordinary columns (one descending: the last member is
    the minimum)"""
    assert B >= 3
    nan = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]
    x = np.zeros((B, 8))
    x[:, 0] = [0.0, -0.0] + [0.0] * (B - 2)
    x[:, 1] = [-0.0, 0.0] + [-0.0] * (B - 2)
    x[:, 2] = [2.5, 2.5, -1.0] + [-1.0] * (B - 3)
    x[:, 3] = [nan] + [float(m) for m in range(1, B)]
    x[:, 4] = [1.0, nan] + [-3.0 - m for m in range(2, B)]
    x[:, 5] = [5e-324, 1e-310] + [0.0] * (B - 2)
    x[:, 6] = [0.1 * (m + 1) * (-1) ** m for m in range(B)]
    x[:, 7] = [float(B - m) for m in range(B)]
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_every_entry_point_is_declared_exported_and_bound():
    decl = _declarations()
    assert sorted(decl) == sorted("rdyhip_ens_" + n for n in NAMES)
    lib = _lib.load()
    for name in decl:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    # the prefixes other files count stay what they were: nothing new begins with them
    bound = [s for s in _lib.SYMBOLS if s.startswith("rdyhip_ens_") and not s.startswith("rdyhip_ens_hr_")]
    assert sorted(bound) == sorted(decl)
    assert lib.rdyhip_version() == 110


def test_argtypes_match_the_header():
    for name, args in _declarations().items():
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args), name
        for text, ct in zip(args, argtypes):
            base = text.replace("const ", "").rsplit(" ", 1)[0].strip()          # "double *", "int32_t", "RDyHipErrorSums *"
            if "*" in text:
                # a pointer in the header is a pointer (or void *) in the table, never a by-value scalar
                assert ct is C.c_void_p or hasattr(ct, "_type_") and not isinstance(ct._type_, str), (name, text, ct)
                if ct is not C.c_void_p and base.startswith("double *") and "**" not in text:
                    assert ct._type_ is C.c_double, (name, text)
                if ct is not C.c_void_p and base.startswith("int32_t"):
                    assert ct._type_ is C.c_int32, (name, text)
                if base.startswith("RDyHipErrorSums"):
                    assert ct._type_ is _lib.RDyHipErrorSums, (name, text)
            else:
                assert ct is CTYPE[base], (name, text, ct)
    assert C.sizeof(_lib.RDyHipErrorSums) == 80


def test_every_entry_point_reports_a_null_operator_first():
    lib = _lib.load()
    i, j, k = C.c_int32(), C.c_int32(), C.c_int32()
    p = _lib.c_double_p()
    v = (C.c_double * 8)()
    ids = (C.c_int32 * 2)()
    s = (_lib.RDyHipErrorSums * 2)()
    calls = {
        "state_planes": (None, 0, None, None, None),                    # every other argument is wrong as well: the operator comes first
        "state_read_begin": (None, 0x7FFFFFFF, None, None),
        "state_read_ready": (None, None),
        "state_read_wait": (None,),
        "state_read_get": (None, -1, 3, -5, None),
        "state_read_ptr": (None, 99, 0, None),
        "error_sums": (None, None, None, None),
        "error_sums_get": (None, None),
        "output_mean_enable": (None, 64),
        "output_mean_accumulate": (None, 99, None, None, None, None),
        "output_mean_get": (None, 3, None, None, None),
        "output_mean_reset": (None, 64, None),
        "output_mean_time": (None, 6, None),
        "series_enable": (None, -1, None, -1),
        "series_record": (None, None, None, None),
        "series_info": (None, None, None, None),
        "series_read": (None, -1, -1, None, None, None),
        "series_clear": (None,),
        "stats": (None, 8, None, None, None),
    }
    assert sorted(calls) == sorted(NAMES)
    for name, args in calls.items():
        assert getattr(lib, "rdyhip_ens_" + name)(*args) == 83, name
        assert b"null operator" in lib.rdyhip_last_error(), (name, lib.rdyhip_last_error())
    # ... and with the other arguments in order
    assert lib.rdyhip_ens_state_read_ready(None, C.byref(i)) == 83 and lib.rdyhip_ens_series_info(None, C.byref(i), C.byref(j), C.byref(k)) == 83
    assert lib.rdyhip_ens_state_read_ptr(None, 0, 1, C.byref(p)) == 83 and lib.rdyhip_ens_error_sums_get(None, s) == 83
    assert lib.rdyhip_ens_series_enable(None, 2, ids, 4) == 83 and lib.rdyhip_ens_series_read(None, 0, 1, v, v, None) == 83


def test_every_kernel_is_in_the_code_object_without_scratch_or_spills():
    """one instantiation of each of the seven kernels; nothing per lane went to scratch, no register was spilled, and a workgroup of
    256 lanes fits a CU; the folds of the error sums use readout_kernels.h's [4 waves][10] doubles of LDS, the streams none"""
    res = codeobj.kernel_resources(build.lib_path())
    families = {"ens_planes_kernel": 0, "ens_error_partial_kernel": 320, "ens_error_finalize_kernel": 320, "ens_output_accumulate_kernel": 0,
                "ens_output_mean_kernel": 0, "ens_series_observe_kernel": 0, "ens_stats_kernel": 0}
    for fam, lds in families.items():
        mine = {k: v for k, v in res.items() if "rdyhip::" + fam in k}
        assert len(mine) == 1, (fam, sorted(mine))
        for k, v in mine.items():
            assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
            assert v["vgpr"] + v["agpr"] <= 256 and v["lds"] == lds, (k, v)
    assert sum("rdyhip::ens_" in k for k in res) == len(families)
    # the kernels of before are all still there, counted the way their own files count them
    assert sum("ensemble_rhs_kernel<" in k for k in res) == 8 and sum("ensemble_hr_kernel<" in k for k in res) == 8
    assert sum("swe_rhs_tiled_kernel<" in k or "swe_rhs_muscl_fused_kernel<" in k for k in res) == 84
    assert sum("swe_rhs_kernel<" in k for k in res) == 4
    for kernel, n in (("state_planes_kernel", 1), ("error_partial_kernel", 1), ("error_finalize_kernel", 1), ("output_accumulate_kernel", 1),
                      ("output_mean_kernel", 2), ("series_observe_kernel", 1), ("series_boundary_record_kernel", 1)):
        assert sum(f"rdyhip::{kernel}" in k for k in res) == n, kernel
    assert sum("tracer_planes_kernel<" in k for k in res) == 14 and sum("tracer_error_" in k for k in res) == 14


def test_the_statistics_rule_on_hand_made_rows():
    B = 4
    x = planted_rows(B)
    mean, lo, hi = ensemble_stats_rule(x)
    pz, nz = _bits(0.0), _bits(-0.0)
    # signed zeros: neither compares below or above the other, member 0's stays -- and the sums are IEEE's: (+0) + (-0) = +0
    assert _bits(lo[0]) == pz and _bits(hi[0]) == pz and _bits(lo[1]) == nz and _bits(hi[1]) == nz
    assert _bits(mean[0]) == pz and _bits(mean[1]) == pz
    # a tie: the value, whichever member's; the mean in member order
    assert hi[2] == 2.5 and lo[2] == -1.0 and mean[2] == ((2.5 + 2.5) + -1.0 + -1.0) * 0.25
    # a NaN in member 0 stays in all three, payload and all in min and max
    assert _bits(lo[3]) == _bits(x[0, 3]) and _bits(hi[3]) == _bits(x[0, 3]) and np.isnan(mean[3])
    # a NaN in a later member is passed over by min and max and poisons the mean only
    assert lo[4] == -6.0 and hi[4] == 1.0 and np.isnan(mean[4])
    # denormals are values like any other
    assert hi[5] == 1e-310 and lo[5] == 0.0 and mean[5] == (5e-324 + 1e-310) * 0.25
    # ordinary columns against numpy's own reductions (the mean against the explicit left-to-right sum)
    for c in (6, 7):
        assert lo[c] == x[:, c].min() and hi[c] == x[:, c].max()
        s = x[0, c]
        for m in range(1, B):
            s = s + x[m, c]
        assert _bits(mean[c]) == _bits(s * (1.0 / B))
    # one member: all three planes are the member, bit for bit (x * 1.0)
    one = ensemble_stats_rule(x[:1])
    assert np.array_equal(_bits(one[1]), _bits(x[0])) and np.array_equal(_bits(one[2]), _bits(x[0]))
    assert np.array_equal(_bits(one[0][[0, 1, 2, 5, 6, 7]]), _bits(x[0][[0, 1, 2, 5, 6, 7]]))
