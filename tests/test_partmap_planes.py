"""csrc/partmap_planes.h on the host: the part map of the LDS-resident match finder as seven bit planes.

The header's two pure functions — 64 part bytes -> 7 x 64 plane bits (k_lz2_partition), and one thread's match bits from its
7 x 4 plane dwords and a part number (lz2_find_part) — against the naive bit loops of tests/partmap_planes_harness.cpp:
all 128 codes at every one of the 64 positions, 10 000 random inputs, every part number 0..126 against random planes and
against planes full of one code (the code 127 of "no position" matches no part).  No GPU: plain g++ against the header alone.
The last test runs the same stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (runtimes linked
statically into the program; nothing is preloaded)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
# 2 backgrounds x 128 codes x 64 positions + 10 000 random; per part: 64 random + 4 uniform + 1 through both functions
CASES = 2 * 128 * 64 + 10000 + 127 * (64 + 4 + 1)


def _compile(tmp, name, *flags):
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe),
                    os.path.join(HERE, "partmap_planes_harness.cpp")], check=True, capture_output=True)
    return str(exe)


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split() == ["ok", str(CASES)], r.stdout[-2000:]


def test_planes_and_match_bits_equal_the_bit_loops(tmp_path):
    _run(_compile(tmp_path, "partmap_planes_harness", "-O2"))


def test_the_same_without_optimisation(tmp_path):
    _run(_compile(tmp_path, "partmap_planes_harness_O0", "-O0"))


def test_under_asan_ubsan(tmp_path):
    exe = _compile(tmp_path, "partmap_planes_harness_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                   "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan")
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
