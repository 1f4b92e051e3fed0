"""bench.py's roofline object (host logic, no GPU): the dominant kernel is credited the job's algorithmic bytes split over its
launches; for whole-buffer Huffman the one-lane heap kernel is reported as latency-bound and the longest
streaming kernel carries the roofline with its own bytes.  --dump-outputs (host logic, and one plain run on the GPU)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dominant_kernel_gets_the_jobs_bytes_per_launch():
    b = _bench()
    n, c, steps, dt = 10**9, 516_875_560, 10, 0.458
    kt = [{"name": "k_lz2_find", "ms": 6.6, "launches": 40}, {"name": "k_lz_parse_emit", "ms": 5.5, "launches": 40}]
    r = b.roofline_of("deflate-h", n, c, kt, steps, dt)
    assert r["kernel"] == "k_lz2_find" and r["launches_per_step"] == 4.0
    assert r["algorithmic_bytes_per_launch"] == (n + c) // 4
    assert abs(r["achieved"] - (n + c) / 4 / 6.6e-3 / 1e9) < 0.01
    assert abs(r["frac"] - r["achieved"] / 8000.0) < 1e-5
    assert abs(r["whole_step_frac"] - (n + c) / (dt / steps) / 1e9 / 8000.0) < 1e-5
    assert "latency_bound" not in r


def test_huffman_heap_kernel_is_not_credited_the_jobs_bytes():
    b = _bench()
    n, c = 10**8, 56_000_000
    kt = [{"name": "k_huff_hist", "ms": 0.08, "launches": 10}, {"name": "k_huff_build", "ms": 0.18, "launches": 10},
          {"name": "k_huff_encode", "ms": 0.15, "launches": 10}]
    r = b.roofline_of("huffman", n, c, kt, 10, 0.0046)
    assert r["kernel"] == "k_huff_encode"
    assert r["algorithmic_bytes_per_launch"] == n + c
    assert abs(r["achieved"] - (n + c) / 0.15e-3 / 1e9) < 0.01
    assert r["latency_bound"]["kernel"] == "k_huff_build" and abs(r["latency_bound"]["ms_per_step"] - 0.18) < 1e-9
    # the whole step still counts both passes over the input
    assert abs(r["whole_step_frac"] - (2 * n + c) / 0.00046 / 1e9 / 8000.0) < 1e-4


def test_no_kernel_times_no_roofline():
    assert _bench().roofline_of("deflate", 1, 1, [], 1, 1.0) is None


def _load(d):
    import numpy as np
    out = {}
    for f in sorted(os.listdir(d)):
        a = np.load(os.path.join(d, f))
        assert f.endswith(".npy") and a.dtype in (np.float32, np.float64), (f, a.dtype)
        out[f[:-4]] = a
    return out


def test_dump_outputs_short_stream_whole_with_its_block_table(tmp_path):
    import types

    import numpy as np
    import torch
    b = _bench()
    data = torch.arange(300, dtype=torch.int64).remainder(256).to(torch.uint8)
    bits = torch.tensor([0, 1000, 2001, 2300], dtype=torch.int64)
    b.dump_outputs(str(tmp_path), types.SimpleNamespace(data=data, block_bits=bits, nbytes=(2300 + 7) // 8), 7)
    got = _load(tmp_path)
    assert set(got) == {"stream_sample", "block_table_bits"}
    assert np.array_equal(got["stream_sample"], data[:288].numpy().astype(np.float32))
    assert np.array_equal(got["block_table_bits"], bits.numpy().astype(np.float64))


def test_dump_outputs_long_stream_is_a_seeded_sample(tmp_path, monkeypatch):
    import types

    import numpy as np
    import torch
    b = _bench()
    monkeypatch.setattr(b, "DUMP_SAMPLE", 64)
    data = torch.randint(0, 256, (5000,), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    h = types.SimpleNamespace(data=data, offsets=torch.tensor([0, 39000], dtype=torch.int64), nbytes=4875)
    runs = []
    for i, seed in enumerate((3, 3, 4)):
        b.dump_outputs(str(tmp_path / str(i)), h, seed)
        runs.append(_load(tmp_path / str(i)))
    pos = torch.randint(0, 4875, (64,), generator=torch.Generator().manual_seed(3)).sort().values
    assert np.array_equal(runs[0]["stream_sample"], data[pos].numpy().astype(np.float32))
    assert np.array_equal(runs[0]["stream_sample"], runs[1]["stream_sample"])
    assert not np.array_equal(runs[0]["stream_sample"], runs[2]["stream_sample"])
    assert np.array_equal(runs[0]["block_table_bits"], [0.0, 39000.0])


def test_dump_outputs_huffman_words_and_code_table(tmp_path):
    import types

    import numpy as np
    import torch
    b = _bench()
    words = torch.tensor([0x04030201, -1, 0x0A], dtype=torch.int32)
    codes, lengths = np.arange(256, dtype=np.uint32) * 0x01010101, np.full(256, 8, np.uint8)
    b.dump_outputs(str(tmp_path), types.SimpleNamespace(words=words, total_bits=70, codes=codes, lengths=lengths), 1)
    got = _load(tmp_path)
    assert np.array_equal(got["stream_sample"], [1, 2, 3, 4, 255, 255, 255, 255, 10])
    assert np.array_equal(got["total_bits"], [70.0]) and np.array_equal(got["codes"], codes.astype(np.float64))
    assert np.array_equal(got["lengths"], lengths.astype(np.float32))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_output(tmp_path):
    """a plain `bench.py` run: the result line with K timed steps, and --dump-outputs holding what lz.compress_h returns
    for the same seeded input"""
    import json
    import subprocess
    import sys

    import numpy as np
    import torch
    from compression_algorithms_amd import lz, synth
    n, seed = 3_000_000, 99
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--bytes", str(n),
                        "--seed", str(seed), "--dump-outputs", str(tmp_path / "out")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("GB/s", True, "u8")
    assert "roofline" not in line and "cpu_baseline" not in line
    got = _load(tmp_path / "out")
    torch.cuda.set_device(0)
    h = lz.compress_h(synth.enwik_like(n, seed=seed, device="cuda:0"), lz.params("deflate"))
    assert line["config"]["compressed_bytes_rank0"] == h.nbytes
    assert np.array_equal(got["block_table_bits"], h.block_bits.cpu().numpy().astype(np.float64))
    assert np.array_equal(got["stream_sample"], h.data[:h.nbytes].cpu().numpy().astype(np.float32))
