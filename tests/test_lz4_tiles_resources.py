"""lz4_tiles' hard limits, read from the bytes that ship (CPU).

The kernel lives on 8 waves per SIMD: 64 VGPRs, no scratch, and
4,976 B of LDS per one-wave workgroup.  A wave now encodes a run of blocks and
carries the next block's 14 prefetched dwords through most of a block, so the
limits are pinned here for both instantiations (aligned / unaligned input),
from the AMDGPU metadata note of the gfx950 code object inside the built
`liblz4jpeg.so`.
"""
import os
import re
import subprocess

import pytest

from test_isa import LIB, _code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
LDS_BYTES = 4976
FIELDS = ("vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")


def _kernel_notes(tmp):
    """{kernel name: {field: int}} of every kernel in the library's gfx950 code objects."""
    kernels = {}
    for k, co in enumerate(_code_objects(LIB)):
        p = tmp / f"co{k}.o"
        p.write_bytes(co)
        text = subprocess.run([READELF, "--notes", str(p)], check=True, capture_output=True,
                              text=True).stdout
        # one YAML map per kernel under amdhsa.kernels, each opening with "  - ."
        for entry in re.split(r"\n  - (?=\.)", text):
            name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
            if not name:
                continue
            vals = {f: int(m.group(1)) for f in FIELDS
                    if (m := re.search(rf"^\s*\.{f}:\s+(\d+)\s*$", entry, re.M))}
            vals["dynamic_stack"] = bool(re.search(r"\.uses_dynamic_stack:\s+true", entry))
            kernels[name.group(1)] = vals
    return kernels


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    if not os.path.exists(LIB) or not os.path.exists(READELF):
        pytest.skip("library not built")
    k = _kernel_notes(tmp_path_factory.mktemp("notes"))
    assert k, "no gfx950 kernel metadata in liblz4jpeg.so"
    return k


@pytest.mark.parametrize("aligned", ["Lb1E", "Lb0E"], ids=["aligned", "unaligned"])
def test_lz4_tiles_keeps_eight_waves_per_simd(notes, aligned):
    names = [n for n in notes if "lz4_tilesI" + aligned in n]
    assert len(names) == 1, (aligned, sorted(notes))
    m = notes[names[0]]
    assert set(FIELDS) <= set(m), m
    # 512 VGPRs per SIMD lane / 8 waves; gfx950 allocates AGPRs from the same file
    assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0 and not m["dynamic_stack"], m
    assert m["group_segment_fixed_size"] == LDS_BYTES, m
    assert m["max_flat_workgroup_size"] == 64, m
