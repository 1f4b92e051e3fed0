"""Resource budget of k_lz2_partition_direct, the partition that keeps its block in registers (CPU only: the kernel is compiled
for gfx950, not run).

Two workgroups of 1 024 threads per CU = eight waves per SIMD.  That takes LDS <= 80 KiB per workgroup, <= 64 VGPRs, and
nothing spilled; the kernel asks the compiler for it with __launch_bounds__(1024, 8).  A change that pushes any of these over
falls back to one workgroup per CU (or to spill code) without a word from the build: this test is where it shows."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compression_algorithms_amd", "csrc")


def _hipcc():
    p = shutil.which("hipcc")
    if p:
        return p
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    p = os.path.join(rocm, "bin", "hipcc")
    return p if os.access(p, os.X_OK) else None


@pytest.fixture(scope="module")
def partition_usage(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("budget") / "lz2_partition.o"
    # the flags of csrc/Makefile, device code only
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-ffp-contract=off",
           "--cuda-device-only", "-c", os.path.join(CSRC, "lz2_partition.hip"), "-o", str(out),
           "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    usage, fn = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            usage[fn] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and fn is not None:
            usage[fn][m.group(1)] = int(m.group(2))
    names = [f for f in usage if "k_lz2_partition_direct" in f]
    assert len(names) == 1, sorted(usage)
    return usage[names[0]]


def test_partition_lds_fits_two_workgroups(partition_usage):
    assert partition_usage["LDS Size"] <= 81920


def test_partition_registers_fit_eight_waves(partition_usage):
    assert partition_usage["VGPRs"] <= 64
    assert partition_usage["AGPRs"] == 0
    assert partition_usage["Occupancy"] >= 8


def test_partition_no_scratch_no_spills(partition_usage):
    assert partition_usage["ScratchSize"] == 0
    assert partition_usage["SGPRs Spill"] == 0
    assert partition_usage["VGPRs Spill"] == 0
