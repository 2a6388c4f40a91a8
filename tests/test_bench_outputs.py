"""bench.py's plain run, --full and --dump-outputs: a plain run measures the
top-level LZ4 line only, --full adds the other lines, and --dump-outputs writes
the last timed step's stream (length, exact chunk sums, head, tail, seeded
sample) as float .npy files that equal the oracle's stream of the same seeded
input and do not change from run to run."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

N = (1 << 20) + 123            # whole blocks + a short last one, 17 dump chunks + a part
NAMES = ("lz4_length", "lz4_stream_chunk_sums", "lz4_stream_head", "lz4_stream_tail",
         "lz4_stream_sample")


def _run(capsys, *argv):
    capsys.readouterr()
    bench.main(["--gpus", "1", "--lz4-bytes-per-rank", str(N)] + list(argv))
    out = capsys.readouterr().out
    lines = [x for x in out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_options_parse_without_a_gpu(capsys, tmp_path):
    bench.main(["--launch-check", "--full", "--dump-outputs", str(tmp_path / "d")])
    assert json.loads(capsys.readouterr().out)["world"] == 1
    assert not (tmp_path / "d").exists()
    with pytest.raises(SystemExit):
        bench.main(["--launch-check", "--steps", "0"])


@pytest.mark.gpu
def test_plain_run_and_dump(gpu, oracle, capsys, tmp_path):
    from lz4jpeg import synth
    d1, d2 = tmp_path / "a", tmp_path / "b"
    line = _run(capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", str(d1))
    assert line["steps"] == 3 and line["warmup"] == 2
    assert line["unit"] == "GB/s" and line["dtype"] == "u8" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] / 1e3) / 1e9, rel=1e-2)
    assert line["roofline"]["avg_launch_ms"] > 0
    for moved in ("jpeg", "lz4_decode", "cfg4_share", "cpu_baseline", "lz4_gather_ms"):
        assert line[moved] is None, moved

    text = synth.random_passages(N, length=30000, seed=1).tobytes()
    ref = np.frombuffer(oracle.lz4_compress(text), dtype=np.uint8)
    assert line["config"]["compressed_bytes_total"] == ref.size
    got = {k: np.load(d1 / f"{k}.npy") for k in NAMES}
    assert sorted(os.listdir(d1)) == sorted(f"{k}.npy" for k in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["lz4_length"].tolist() == [ref.size]
    pad = np.zeros(-ref.size % 65536, np.uint8)
    chunks = np.concatenate([ref, pad]).reshape(-1, 65536).astype(np.int64)
    sums = np.stack([chunks.sum(1), (chunks * np.arange(1, 65537)).sum(1)], 1)
    assert np.array_equal(got["lz4_stream_chunk_sums"], sums.astype(np.float64))
    assert np.array_equal(got["lz4_stream_head"], ref[:1 << 20].astype(np.float32))
    assert np.array_equal(got["lz4_stream_tail"], ref[-(1 << 20):].astype(np.float32))
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, ref.size, 1 << 22))
    assert np.array_equal(got["lz4_stream_sample"], ref[idx].astype(np.float32))

    # the same arguments again: the same files
    _run(capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", str(d2))
    for k in NAMES:
        assert np.array_equal(got[k], np.load(d2 / f"{k}.npy")), k


@pytest.mark.gpu
def test_full_run_adds_the_other_lines(gpu, capsys):
    line = _run(capsys, "--steps", "2", "--warmup", "1", "--full", "--no-cfg4-share",
                "--no-jpeg-batch", "--no-cpu-baseline", "--jpeg-w", "64", "--jpeg-h", "48")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["lz4_decode"]["roundtrip_ok"] is True
    assert line["lz4_decode"]["bare_stream"]["roundtrip_ok"] is True
    assert line["jpeg"]["value"] > 0 and line["jpeg"]["reconstruct"]["value"] > 0
    assert line["jpeg"]["entropy"]["roundtrip_ok"] is True
