"""lz4_emit's hard limits, read from the bytes that ship (CPU).

The kernel runs four 8-wave workgroups per CU, the wave-slot limit (DESIGN
4.2): at most 64 VGPRs, no spills, no scratch, and at most 40,960 B of LDS
(160 KB / 4).  Whatever a change to its sequence rounds or its literal pass
keeps per round or per workgroup must not cost that occupancy; pinned here
from the AMDGPU metadata note of the gfx950 code object inside the built
`liblz4jpeg.so`.
"""
import os

import pytest

from test_isa import LIB
from test_lz4_tiles_resources import FIELDS, READELF, _kernel_notes

LDS_MAX = 40960


@pytest.fixture(scope="module")
def emit_notes(tmp_path_factory):
    if not os.path.exists(LIB) or not os.path.exists(READELF):
        pytest.skip("library not built")
    k = _kernel_notes(tmp_path_factory.mktemp("emit_notes"))
    assert k, "no gfx950 kernel metadata in liblz4jpeg.so"
    return k


def test_lz4_emit_keeps_four_workgroups_per_cu(emit_notes):
    names = [n for n in emit_notes if "lz4_emit" in n]
    assert len(names) == 1, sorted(emit_notes)
    m = emit_notes[names[0]]
    assert set(FIELDS) <= set(m), m
    # 512 VGPRs per SIMD lane / 8 waves; gfx950 allocates AGPRs from the same file
    assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0 and not m["dynamic_stack"], m
    assert 0 < m["group_segment_fixed_size"] <= LDS_MAX, m
    assert m["max_flat_workgroup_size"] == 512, m
