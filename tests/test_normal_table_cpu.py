"""The host pass of the normal table (rdycore_amd/csrc/normal_table.h: the distinct (stored component, CS_IS_CN, OTHER_NEG)
triples of the tile edge records, their indices in bits 26-31 of the records' words), checked without a GPU: the device-free
header is compiled into a small stand-alone program (tests/host/normal_table_test.cpp) under the address and
undefined-behaviour sanitizers, with their runtimes linked in, and the program is run directly -- never loaded into Python.

It prints one PASS / FAIL line per check: no records; 1, 6, exactly 64 keys (a table) and 65 (streamed, every word untouched,
also when the 65th key is the last record's); +0.0 / -0.0 and equal components under different flag bits as different keys;
boundary and not-owned records; bits 0-25 of every word unchanged and every record's entry reproducing its own pair."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "normal_table_test.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

CHECKS = ["no_records", "keys_1", "keys_6", "keys_64", "keys_65_is_streamed_and_untouched", "keys_200_is_streamed_and_untouched",
          "late_65th_key_leaves_every_word_untouched", "entries_in_order_of_first_appearance", "plus_and_minus_zero_are_two_keys",
          "equal_cs_with_different_flags_are_different_keys", "boundary_records_share_the_keys", "occupied_high_bits_mean_streamed",
          "nan_payloads_are_patterns"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("normal_table")), "normal_table_test")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx] + FLAGS + static + [f"-I{ROOT}/rdycore_amd/csrc", "-o", exe, SOURCE])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stdout + out.stderr        # a sanitizer report ends the program with its own status
    assert out.stderr == "", out.stderr
    lines = [ln.split() for ln in out.stdout.strip().split("\n")]
    assert lines[-1] == ["0", "failure(s)"]
    return {name: verdict for verdict, name in lines[:-1]}


def test_the_header_includes_nothing_of_the_device():
    text = open(os.path.join(ROOT, "rdycore_amd", "csrc", "normal_table.h")).read()
    includes = [ln.split()[1] for ln in text.split("\n") if ln.startswith("#include")]
    assert includes and all("hip" not in i for i in includes), includes
    assert [i for i in includes if not i.startswith("<")] == ['"tile_format.h"'], includes


@pytest.mark.parametrize("name", CHECKS)
def test_host_pass(report, name):
    assert report.get(name) == "PASS", name


def test_nothing_the_program_checks_goes_unasserted(report):
    assert sorted(report) == sorted(CHECKS)


def test_the_index_bits_are_free_in_the_record_word():
    """tile_format.h: every field of a packed record lies in bits 0-25, the table has as many entries as six bits address, and
    the LDS of the table kernels is the streamed kernels' plus 64 pairs of doubles"""
    text = open(os.path.join(ROOT, "rdycore_amd", "csrc", "tile_format.h")).read()
    shifts = [int(s) for s in re.findall(r"constexpr uint32_t EDGE_\w+\s*=\s*1u << (\d+);", text)]
    assert shifts and max(shifts) == 25, shifts
    assert re.search(r"constexpr int\s+NORMAL_TABLE_MAX\s*=\s*64;", text) and re.search(r"constexpr int\s+EDGE_NT_SHIFT\s*=\s*26;", text)
    assert "tiled_lds_bytes(S, hr) + 2 * sizeof(double) * (size_t)NORMAL_TABLE_MAX" in text


def test_the_off_switch_is_a_config_bit_with_a_python_mirror():
    header = open(os.path.join(ROOT, "include", "rdyhip.h")).read()
    assert re.search(r"#define RDYHIP_CONFIG_STREAMED_NORMALS 2\b", header)
    assert "int rdyhip_normal_table_info(RDyHipOperator op, int32_t *entries, int32_t *active);" in header
    from rdycore_amd.operator import RDyFlowConfig
    assert RDyFlowConfig().streamed_normals is False
