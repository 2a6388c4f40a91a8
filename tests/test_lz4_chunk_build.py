"""The small-chunk test build of the compressor (`make chunk12`, part of
`make all`): it exists, holds the compressor's entry points, is built with the
product's flags plus the one define, and says so (no GPU: nothing is launched).
"""
import os
import subprocess

import pytest

import lz4_chunk_lib

REPO = lz4_chunk_lib.REPO


def _make(*args):
    return subprocess.run(["make", "-s", "-C", REPO, *args], check=True, capture_output=True,
                          text=True).stdout


def _make_var(name):
    return _make(f"print-{name}").split()


def test_variant_is_built_and_exports_the_compressor():
    assert os.path.exists(lz4_chunk_lib.CHUNK12_PATH), \
        f"run `make {lz4_chunk_lib.CHUNK12_TARGET}` (part of `make all`)"
    out = subprocess.run(["nm", "-D", "--defined-only", lz4_chunk_lib.CHUNK12_PATH],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = set(lz4_chunk_lib.COMPRESSOR_ENTRY_POINTS) - exported
    assert not missing, missing
    # self-contained: nothing of the project is left undefined
    out = subprocess.run(["nm", "-D", "--undefined-only", lz4_chunk_lib.CHUNK12_PATH],
                         capture_output=True, text=True, check=True).stdout
    undefined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    assert not {u for u in undefined if u.startswith(("lz4r", "lz4_", "jpegr", "lz4jpeg"))}


def test_variant_flags_are_the_products_plus_one_define():
    flags = _make_var("CHUNK12_HIPFLAGS")
    define = f"-DLZ4R_CHUNK_LOG2={lz4_chunk_lib.CHUNK12_LOG2}"
    assert _make_var("CHUNK12_DEFINE") == [define]
    assert flags == _make_var("HIPFLAGS") + _make_var("LZ4R_HIPFLAGS") + [define]
    assert "--offload-arch=gfx950" in flags and "-amdgpu-sched-strategy=max-ilp" in flags
    # the rule compiles lz4r.hip alone with exactly these flags into the library
    lib = os.path.relpath(lz4_chunk_lib.CHUNK12_PATH, REPO)
    assert _make_var("CHUNK12_LIB") == [lib]
    recipe = subprocess.run(["make", "-n", "-B", "-C", REPO, lib], check=True, capture_output=True,
                            text=True).stdout
    line = [l.split() for l in recipe.splitlines() if "hipcc" in l and lib in l]
    assert len(line) == 1, recipe
    words = line[0]
    assert words[1:1 + len(flags)] == flags, words
    assert words[1 + len(flags):] == ["-shared", "-o", lib, "lz4-jpeg_amd/csrc/lz4r.hip"], words


def test_variant_depends_on_the_headers_of_lz4r_o():
    targets = (os.path.relpath(lz4_chunk_lib.CHUNK12_PATH, REPO), "lz4-jpeg_amd/build/lz4r.o")
    # make's database after it has looked both targets up (nothing is built)
    db = subprocess.run(["make", "-pnq", "-C", REPO, *targets], capture_output=True,
                        text=True).stdout
    deps = {}
    for target in targets:
        rule = [l for l in db.splitlines() if l.startswith(target + ": ") and "=" not in l]
        assert rule, target
        deps[target] = {d for d in rule[0].split(":", 1)[1].split() if d.endswith(".h")}
    a, b = deps.values()
    assert a == b and "lz4-jpeg_amd/csrc/lz4r_tiles.h" in a and "include/lz4r.h" in a


def test_both_builds_report_their_chunk():
    assert lz4_chunk_lib.chunk_blocks("chunk12") == 1 << 12
    assert lz4_chunk_lib.chunk_blocks("product") == 1 << 24
    for name in lz4_chunk_lib.NAMES:
        assert lz4_chunk_lib.chunk_blocks(name) == lz4_chunk_lib.expected_chunk_blocks(name)
        L = lz4_chunk_lib.load(name)
        assert L.lz4r_nblocks(301) == 2 and L.lz4r_compress_bound(600) == 1 + 2 * 1152


def test_missing_variant_is_an_error_naming_the_target(monkeypatch, tmp_path):
    monkeypatch.setattr(lz4_chunk_lib, "_loaded", {})
    monkeypatch.setattr(lz4_chunk_lib, "CHUNK12_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(lz4_chunk_lib.VariantMissing, match="make .*chunk12"):
        lz4_chunk_lib.load("chunk12")
