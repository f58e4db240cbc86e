"""Phase 2 of the tiled kernels' tile loop -- the per-cell sum behind the second barrier -- reads LDS in one batch: the wave
speeds and fluxes of all slots and the lane's own depth and velocities are issued together and waited for once, where the commit
before read them one guard at a time.  Counted in the machine code, without a GPU, with the tool and the compile of
tests/test_normal_table_isa_cpu.py: tools/isa_hot_loop.phase2_round_trips looks at the hot loop from its second s_barrier to the
first hinted global_load behind it (the next tile's per-cell streams) and counts the s_waitcnt instructions that carry an
lgkmcnt and have at least one ds_read issued since the previous such wait -- the LDS round trips a wave pays in series there
(static: the cold Courant tie path included).

                                                streamed    table
  the commit before (PARENT_ROUND_TRIPS)          16          16     (slots 2 + 4 + 4, tie path 3, own cell 3)
  this build, measured                            2           2      (the batch; the own momenta, read where the friction term
                                                                      uses them -- swe_tiled_body.h says why)"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "ILi3ELi0ELb1ELb0ELb0ELb1E"
KERNELS = {"streamed": "swe_rhs_tiled_kernel" + ARGS, "table": "swe_rhs_ntab_kernel" + ARGS}
PARENT_ROUND_TRIPS = {"streamed": 16, "table": 16}     # tools/isa_hot_loop.phase2_round_trips on the commit before
MEASURED_ROUND_TRIPS = {"streamed": 2, "table": 2}


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hot_loop
    d = tmp_path_factory.mktemp("phase2_round_trips")
    src, asm = str(d / "both.hip"), str(d / "both.s")
    sig = "(const rdyhip::KernelArgs, const double, const double *, double *);\n"
    with open(src, "w") as fh:
        fh.write('#include "swe_kernels.h"\n'
                 "template __global__ void rdyhip::swe_rhs_tiled_kernel<3, 0, true, false, false, true>" + sig +
                 "template __global__ void rdyhip::swe_rhs_ntab_kernel<3, 0, true, false, false, true>" + sig)
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           f"-I{ROOT}/include", f"-I{ROOT}/rdycore_amd/csrc", "-o", asm, src], stderr=subprocess.DEVNULL)
    return isa_hot_loop, open(asm).read().split("\n")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
@pytest.mark.parametrize("family", sorted(KERNELS))
def test_phase_2_pays_at_least_seven_lds_round_trips_fewer_than_the_commit_before(both, family):
    tool, lines = both
    n = tool.phase2_round_trips(lines, KERNELS[family])
    print(f"{family}: {n} LDS round trips in phase 2 (the commit before: {PARENT_ROUND_TRIPS[family]})")
    assert n <= MEASURED_ROUND_TRIPS[family] + 1, n
    assert n <= PARENT_ROUND_TRIPS[family] - 7, n


def test_the_counter_counts_waits_that_follow_a_read():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hot_loop
    code = ["ds_read_b64 v[0:1], v2", "s_waitcnt lgkmcnt(0)", "s_waitcnt lgkmcnt(0)", "ds_read_b64 v[0:1], v2", "ds_read_b64 v[4:5], v2",
            "s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(1)", "s_waitcnt lgkmcnt(0)", "s_load_dword s0, s[2:3], 0x0", "s_waitcnt lgkmcnt(0)",
            "ds_read_b64 v[0:1], v2", "s_waitcnt vmcnt(0) lgkmcnt(0)"]
    assert isa_hot_loop.lds_round_trips(code) == 3
