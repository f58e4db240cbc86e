"""The host-side rules of the uniform fields (rdycore_amd/csrc/uniform_fields.h: which writes start, keep and end the mode in
which the first-order / HR kernels read element 0 of the water source, of Manning's n or of the bed slopes), checked without a
GPU: the device-free header is compiled into a small stand-alone program (tests/host/uniform_fields_check.cpp) under the address
and undefined-behaviour sanitizers, with their runtimes linked in, and the program is run directly -- never loaded into Python.

It prints one PASS / FAIL line per check: the scan on arrays that differ only in their last or only in their first element,
+0.0 / -0.0 mixed, equal and unequal NaNs, n = 1 and n = 0 -- below and above the size from which the scan runs in pieces --
and every transition of the rules of include/rdyhip.h ("Uniform fields"), in sequence."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "uniform_fields_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

SCAN = ["scan_uniform", "scan_last_differs", "scan_first_differs", "scan_middle_differs", "scan_plus_zero", "scan_mixed_zeros",
        "scan_minus_zero", "scan_equal_nans", "scan_unequal_nans"]
TRANSITIONS = ["create_all_uniform_plus_zero", "source_bit_needs_water_only", "create_sloped_bed", "whole_write_starts",
               "whole_write_restarts_with_new_value", "partial_write_of_the_value_keeps", "partial_fill_of_the_value_keeps",
               "partial_write_of_another_value_ends", "partial_write_does_not_start", "partial_fill_does_not_start",
               "whole_write_of_unequal_values_stays_off", "whole_fill_starts", "partial_fill_of_another_value_ends",
               "whole_write_of_unequal_values_ends", "unseen_write_ends", "partial_write_after_end_stays_off",
               "whole_write_restarts_after_end", "minus_zero_is_not_plus_zero", "escape_ends", "escape_is_for_good",
               "other_fields_are_untouched", "disabled_stays_off"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("uniform_fields")), "uniform_fields_check")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx] + FLAGS + static + [f"-I{ROOT}/rdycore_amd/csrc", "-o", exe, SOURCE])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stdout + out.stderr        # a sanitizer report ends the program with its own status
    assert out.stderr == "", out.stderr
    lines = [ln.split() for ln in out.stdout.strip().split("\n")]
    assert lines[-1] == ["0", "failure(s)"]
    return {name: verdict for verdict, name in lines[:-1]}


def test_the_header_includes_nothing_of_the_device():
    text = open(os.path.join(ROOT, "rdycore_amd", "csrc", "uniform_fields.h")).read()
    includes = [ln.split()[1] for ln in text.split("\n") if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


@pytest.mark.parametrize("size", ["small", "pieces"])
def test_scan_compares_bit_patterns_and_sees_either_end(report, size):
    for name in SCAN:
        assert report.get(f"{name}_{size}") == "PASS", name


def test_scan_edge_sizes_and_strides(report):
    for name in ("scan_n1", "scan_n0", "all_have_pattern_n0", "scan_stride3", "scan_stride3_last_differs", "bed_is_flat"):
        assert report.get(name) == "PASS", name


def test_every_transition_in_sequence(report):
    for name in TRANSITIONS:
        assert report.get(name) == "PASS", name
    # nothing the program checks goes unasserted here
    assert len(report) == 2 * len(SCAN) + 6 + len(TRANSITIONS)
