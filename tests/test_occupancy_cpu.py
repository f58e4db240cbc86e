"""Workgroups per CU of the first-order / HR tiled kernels, checked on the built library without a GPU.

A (S, SRC, HR) family runs all six of its OVERWRITE / EULER / FNT instantiations on ONE persistent grid, sized at create from
the family's setting (tiled_blocks_per_cu, swe_kernels.h; rdyhip_tiled_workgroups_per_cu reports it).  A family set to four
must fit four times in a CU with every instantiation: a workgroup is one wave on each SIMD, four workgroups are four waves per
SIMD = at most 128 of its 512 VGPRs each, and four times the dynamic LDS the host asks for within the CU's 160 KiB.  One
register more in one of the six and the hardware places three where the grid was sized for four: the fourth waits for a slot
and its tiles run as a tail.  Both lists are explicit: a family that changes its setting fails here until the list (and the
A/B timing behind it, profiles/RESULTS_LOG.md section 15) follows."""
import itertools
import re

import pytest

from rdycore_amd import _lib, build, codeobj
from rdycore_amd import mesh as M
from rdycore_amd.operator import RDyFlowConfig, probe_layout

# (slots per cell, source method, hydrostatic reconstruction)
FOUR = [(3, 0, False)]
THREE = [(3, 0, True), (3, 1, False), (3, 1, True), (4, 0, False), (4, 0, True), (4, 1, False), (4, 1, True)]
LDS_PER_CU = 160 * 1024
RX = re.compile(r"swe_rhs_tiled_kernel<(\d), (\d), (true|false), (true|false), (true|false), (true|false)>")


def _family_kernels():
    fam = {}
    for name, r in codeobj.kernel_resources(build.lib_path()).items():
        m = RX.search(name)
        if m:
            fam.setdefault((int(m.group(1)), int(m.group(2)), m.group(4) == "true"), {})[name] = r
    return fam


def _lds_requested(S, src, hr):
    mesh = M.structured_tri_mesh(24, 20) if S == 3 else M.structured_quad_mesh(40, 30)
    return probe_layout(RDyFlowConfig(source_method=src, well_balancing=2 if hr else 0), mesh)["lds_bytes"]


def test_every_family_is_listed_with_its_setting():
    assert sorted(FOUR + THREE) == sorted(itertools.product((3, 4), (0, 1), (False, True)))
    fam = _family_kernels()
    assert sorted(fam) == sorted(FOUR + THREE) and all(len(v) == 6 for v in fam.values())      # 8 families x 6 = 48
    q = _lib.load().rdyhip_tiled_workgroups_per_cu
    got = {f: q(f[0], f[1], int(f[2])) for f in FOUR + THREE}
    assert got == {**{f: 4 for f in FOUR}, **{f: 3 for f in THREE}}, got
    assert q(5, 0, 0) == 0 and q(3, 2, 0) == 0


@pytest.mark.parametrize("family", FOUR, ids=str)
def test_a_family_at_four_fits_four_times_with_all_six_instantiations(family):
    kernels = _family_kernels()[family]
    assert len(kernels) == 6
    bad = {k: r for k, r in kernels.items() if r["vgpr"] + r["agpr"] > 128 or r["scratch"] != 0 or r["vgpr_spills"] != 0}
    assert not bad, bad
    lds = _lds_requested(*family)
    static = max(r["lds"] for r in kernels.values())             # static LDS of a kernel comes on top of the dynamic block
    assert lds > 0 and 4 * (lds + static) <= LDS_PER_CU, (lds, static)


@pytest.mark.parametrize("family", THREE, ids=str)
def test_a_family_at_three_fits_three_times(family):
    kernels = _family_kernels()[family]
    assert all(r["vgpr"] + r["agpr"] <= 168 and r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in kernels.values()), kernels
    assert 0 < 3 * (_lds_requested(*family) + max(r["lds"] for r in kernels.values())) <= LDS_PER_CU
