"""Resource budget of k_lz2_find, the per-part match finder (CPU only: the kernel is compiled for gfx950, not run).

Four workgroups of 512 threads per CU = eight waves per SIMD.  That takes LDS <= 40 KiB per workgroup, <= 64 VGPRs and
<= 80 SGPRs, and nothing spilled; the kernel asks the compiler for it with __launch_bounds__(512, 8).  A change that
pushes any of these over falls back to three workgroups per CU (or to spill code) without a word from the build: this
test is where it shows."""
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
def find_usage(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("budget") / "lz2_find.o"
    # the flags of csrc/Makefile, device code only
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-ffp-contract=off",
           "--cuda-device-only", "-c", os.path.join(CSRC, "lz2_find.hip"), "-o", str(out),
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
    names = [f for f in usage if re.fullmatch(r"_Z10k_lz2_findPK.*", f)]
    assert len(names) == 1, sorted(usage)
    return usage[names[0]]


def test_find_lds_fits_four_workgroups(find_usage):
    assert find_usage["LDS Size"] <= 40960


def test_find_registers_fit_eight_waves(find_usage):
    assert find_usage["VGPRs"] <= 64
    assert find_usage["AGPRs"] == 0
    assert find_usage["TotalSGPRs"] <= 80
    assert find_usage["Occupancy"] >= 8


def test_find_no_scratch_no_spills(find_usage):
    assert find_usage["ScratchSize"] == 0
    assert find_usage["SGPRs Spill"] == 0
    assert find_usage["VGPRs Spill"] == 0
