"""csrc/lz_plan.h on the host: how a call of the 64 KiB-block encoder decides how to run — batch size, overlap, where the odd
batches' fallback chains go, the fallback grids, stage B's launch shape — as a pure function of (blocks, CUs, the fallback hint,
the environment switches), and how the switches are parsed.  No GPU: tests/lz_plan_harness.cpp is compiled with plain g++
against that header alone.

The rules are restated here from DESIGN.md (§3 "Data layout", §4.3's rows on the batch rule, the second fallback stream and the
fallback grids, §4.9) and from the comments that travel with them — not derived from the header."""
import os
import random
import subprocess
from collections import namedtuple

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# the order of lz_plan_harness.cpp's print_switches; the last three exist in a -DMI_MEASURE build only
SW = namedtuple("SW", "v2 batch no_overlap b_split fb2_side prof rows rows_waves big_split lanes_kib prefix debug sliced serial "
                      "skip stop_phase no_fb")
DEFAULT = SW(v2=1, batch=0, no_overlap=0, b_split=1, fb2_side=-1, prof=0, rows=1, rows_waves=9, big_split=1, lanes_kib=8, prefix=1,
             debug=0, sliced=1, serial=0, skip=0, stop_phase=0, no_fb=0)
ENV = {"v2": "MI_LZ_V2", "batch": "MI_LZ_BATCH", "no_overlap": "MI_LZ_NO_OVERLAP", "b_split": "MI_LZ_B_SPLIT",
       "fb2_side": "MI_LZ_FB2_SIDE", "prof": "MI_LZ_PROF_FALLBACK", "rows": "MI_LZ_ROWS", "rows_waves": "MI_LZ_ROWS_WAVES",
       "big_split": "MI_LZ_BIG_SPLIT", "lanes_kib": "MI_LZ_LANES_KIB", "prefix": "MI_LZ_PREFIX", "debug": "MI_LZ_DEBUG",
       "sliced": "MI_LZW_SLICED", "serial": "MI_LZS_SERIAL", "skip": "MI_LZ_SKIP", "stop_phase": "MI_LZ_STOP_PHASE",
       "no_fb": "MI_LZ_UNSAFE_NO_FALLBACK"}
MEASURE_ONLY = ("skip", "stop_phase", "no_fb")

LZ_FB_GRID = 128
ODD_FB, ODD_FB2, ODD_STAGE_B = 0, 1, 2
B_ROWS_SPLIT, B_SPLIT, B_ONE = 0, 1, 2


def _compile(tmp, name, *flags):
    exe = tmp / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-o", str(exe), os.path.join(HERE, "lz_plan_harness.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("lz_plan"), "lz_plan_harness")


@pytest.fixture(scope="module")
def harness_measure(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("lz_plan_measure"), "lz_plan_harness_measure", "-DMI_MEASURE")


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------
def batch_blocks(nblocks, fb, of, sw):
    if sw.batch:                                              # MI_LZ_BATCH wins over both rules
        cap = sw.batch
    elif fb > 8 and fb * 16 >= of:                            # the input lives in the fallback pipeline: the old rule
        cap = 1024 if nblocks < 6144 else 2048 if nblocks < 9216 else 3072
    else:                                                     # as few, as large and as equal batches as fit 3 840 blocks
        nbat = -(-nblocks // 3840)
        cap = -(-nblocks // nbat) if nbat else 1
    return max(1, min(nblocks, cap))


def grids(nb, num_cu, fb, sw):
    if not sw.v2:                                             # the first pipeline for every block: no list, no hint
        return (LZ_FB_GRID, nb, 1024, min(nb, 1024), 0)
    fb_want = max(fb, LZ_FB_GRID)
    cap = 512 if fb > LZ_FB_GRID else LZ_FB_GRID
    small = min(2 * nb, 6 * num_cu) if fb > 8 else 0
    return (fb_want, min(nb, fb_want), cap, min(nb, cap), small)


def plan(nblocks, num_cu, fb, of, sw, measure=False):
    nbmax = batch_blocks(nblocks, fb, of, sw)
    overlap = nblocks > nbmax and not sw.no_overlap
    skip = sw.skip if measure else 0
    solo = (not overlap) and bool(sw.b_split) and bool(sw.v2) and not skip      # a call of one batch runs solo
    busy = overlap and fb > 8                                 # without overlap: never busy
    if not busy:
        chain, want_fb2 = ODD_FB, False
    else:
        side = (sw.fb2_side == 1) if sw.fb2_side >= 0 else fb * 2 >= of
        chain, want_fb2 = (ODD_STAGE_B, False) if side else (ODD_FB2, True)
    shape = B_ONE if not sw.big_split else B_ROWS_SPLIT if sw.rows else B_SPLIT
    tail = nblocks % nbmax or nbmax
    return (nbmax, int(overlap), 3 if overlap else 1, int(solo), int(busy), chain, int(want_fb2), shape, skip,
            int(bool(sw.no_fb)) if measure else 0) + grids(nbmax, num_cu, fb, sw) + grids(tail, num_cu, fb, sw)


FIELDS = ("nbmax overlap nsets solo fb_busy odd_chain want_fb2 b_shape skip no_fallback fb_want fgrid giant_cap giant_grid small_grid "
          "tail_fb_want tail_fgrid tail_giant_cap tail_giant_grid tail_small_grid").split()


def run_plans(harness, tmp_path, cases):
    """cases: (nblocks, num_cu, fb, of, SW) -> the harness's tuples"""
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for nblocks, num_cu, fb, of, sw in cases:
            f.write(" ".join(str(v) for v in (nblocks, num_cu, fb, of) + tuple(sw)) + "\n")
    r = subprocess.run([harness, "plan", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == len(cases)
    return got


def one(harness, tmp_path, nblocks, fb=0, of=0, num_cu=256, **sw):
    return dict(zip(FIELDS, run_plans(harness, tmp_path, [(nblocks, num_cu, fb, of, DEFAULT._replace(**sw))])[0]))


def other_settings(measure):
    out = [DEFAULT]
    for k, v in dict(v2=0, no_overlap=1, b_split=0, prof=1, rows=0, rows_waves=4, big_split=0, lanes_kib=16, prefix=0, debug=1, sliced=0,
                     serial=1).items():
        out.append(DEFAULT._replace(**{k: v}))
    out += [DEFAULT._replace(batch=b) for b in (1, 64, 1024, 4096)]
    out += [DEFAULT._replace(fb2_side=0), DEFAULT._replace(fb2_side=1)]
    out += [DEFAULT._replace(rows=0, big_split=0), DEFAULT._replace(v2=0, b_split=0, no_overlap=1)]
    if measure:
        out += [DEFAULT._replace(skip=s) for s in (1, 2, 3)] + [DEFAULT._replace(no_fb=1), DEFAULT._replace(stop_phase=3)]
    return out


NBLOCKS = [0, 1, 2, 3839, 3840, 3841, 6143, 6144, 9215, 9216, 15259, 40000]
FB = [0, 8, 9, 128, 129, 600]
OF = [0, 16, 143, 144, 145, 1024, 3815]


def _sweep(harness, tmp_path, nblocks_list, measure):
    cases = [(nb, 256, fb, of, sw) for nb in nblocks_list for fb in FB for of in OF for sw in other_settings(measure)]
    got = run_plans(harness, tmp_path, cases)
    for case, g in zip(cases, got):
        want = plan(*case, measure=measure)
        assert g == want, (case, dict(zip(FIELDS, g)), dict(zip(FIELDS, want)))


def test_plan_equals_the_restated_rules(harness, tmp_path):
    rng = random.Random(20260119)
    seeded = [rng.randrange(1, 50000) for _ in range(200)] + [rng.randrange(1, 12000) for _ in range(100)]
    _sweep(harness, tmp_path, NBLOCKS + seeded, measure=False)


def test_plan_of_a_measurement_build(harness_measure, tmp_path):
    _sweep(harness_measure, tmp_path, NBLOCKS, measure=True)


# ---- known answers from the code's own comments -------------------------------------------------------------------------------------
def test_batches_of_the_measured_sizes(harness, tmp_path):
    p = one(harness, tmp_path, 1526)                          # 10^8 B: one batch, no pipeline
    assert (p["nbmax"], p["overlap"], p["nsets"], p["solo"]) == (1526, 0, 1, 1)
    assert one(harness, tmp_path, 4578)["nbmax"] == 2289      # 3 x 10^8 B: 2 x 2 289
    assert one(harness, tmp_path, 7630)["nbmax"] == 3815      # 5 x 10^8 B: 2 x 3 815
    p = one(harness, tmp_path, 15259)                         # 10^9 B: 4 x 3 815
    assert (p["nbmax"], p["overlap"], p["nsets"], p["solo"]) == (3815, 1, 3, 0)


@pytest.mark.parametrize("nblocks,old", [(6143, 1024), (6144, 2048), (9215, 2048), (9216, 3072), (9217, 3072), (15259, 3072)])
def test_the_old_batch_rule_for_input_that_lives_in_the_fallback(harness, tmp_path, nblocks, old):
    new = one(harness, tmp_path, nblocks)["nbmax"]
    assert new == -(-nblocks // -(-nblocks // 3840))                          # (equal to the old rule's at 9 216 = 3 x 3 072 only)
    assert one(harness, tmp_path, nblocks, fb=9, of=144)["nbmax"] == old      # a sixteenth of the batch: the old rule
    assert one(harness, tmp_path, nblocks, fb=9, of=145)["nbmax"] == new      # less than a sixteenth
    for of in OF:
        assert one(harness, tmp_path, nblocks, fb=8, of=of)["nbmax"] == new   # 8 blocks are not "more than 8"


def test_batch_switch_bounds(harness, tmp_path):
    # the plan takes what lz_switches_read() took: 1 and 4096 are, 0 and 4097 are not
    for value, batch in (("1", 1), ("4096", 4096), ("0", 0), ("4097", 0)):
        assert _switches(harness, {"MI_LZ_BATCH": value})["batch"] == batch
    assert one(harness, tmp_path, 15259, batch=1)["nbmax"] == 1
    assert one(harness, tmp_path, 15259, batch=4096)["nbmax"] == 4096
    assert one(harness, tmp_path, 15259, batch=0)["nbmax"] == 3815
    assert one(harness, tmp_path, 15259, fb=600, of=1024, batch=64)["nbmax"] == 64


def test_where_the_odd_chains_go(harness, tmp_path):
    n = 15259
    p = one(harness, tmp_path, n, fb=600, of=1024)            # most blocks fall back: stage B's stream, no second stream
    assert (p["fb_busy"], p["odd_chain"], p["want_fb2"]) == (1, ODD_STAGE_B, 0)
    p = one(harness, tmp_path, n, fb=512, of=1024)            # fb * 2 == of: still stage B's
    assert (p["odd_chain"], p["want_fb2"]) == (ODD_STAGE_B, 0)
    p = one(harness, tmp_path, n, fb=511, of=1024)            # stage B has work of its own: a second stream
    assert (p["fb_busy"], p["odd_chain"], p["want_fb2"]) == (1, ODD_FB2, 1)
    p = one(harness, tmp_path, n, fb=8, of=16)                # not busy
    assert (p["fb_busy"], p["odd_chain"], p["want_fb2"]) == (0, ODD_FB, 0)
    p = one(harness, tmp_path, n, fb=600, of=1024, fb2_side=0)
    assert (p["odd_chain"], p["want_fb2"]) == (ODD_FB2, 1)
    p = one(harness, tmp_path, n, fb=9, of=3815, fb2_side=1)
    assert (p["odd_chain"], p["want_fb2"]) == (ODD_STAGE_B, 0)
    p = one(harness, tmp_path, n, fb=8, of=16, fb2_side=1)    # the switch forces a side, not business
    assert (p["fb_busy"], p["odd_chain"], p["want_fb2"]) == (0, ODD_FB, 0)
    for kw in (dict(no_overlap=1), dict()):                   # without overlap — switched off, or a call of one batch — never busy
        p = one(harness, tmp_path, n if kw else 1000, fb=600, of=1024, **kw)
        assert (p["overlap"], p["fb_busy"], p["odd_chain"], p["want_fb2"]) == (0, 0, ODD_FB, 0)


def test_fallback_grids(harness, tmp_path):
    nb = 3815
    for fb in (0, 8, 9, 128, 129, 600):
        p = one(harness, tmp_path, 15259, fb=fb, of=3815, batch=nb)           # (the batch held: the old rule would change it)
        assert p["nbmax"] == nb
        assert p["fb_want"] == max(fb, LZ_FB_GRID)
        assert p["fgrid"] == max(fb, LZ_FB_GRID)
        assert p["giant_cap"] == (512 if fb > LZ_FB_GRID else LZ_FB_GRID)
        assert p["small_grid"] == (6 * 256 if fb > 8 else 0)
    p = one(harness, tmp_path, 100, fb=600, of=1024)          # a small batch: min(2 nb, 6 CUs), every block its workgroup
    assert (p["fgrid"], p["giant_grid"], p["small_grid"]) == (100, 100, 200)
    p = one(harness, tmp_path, 15259, fb=600, of=1024, v2=0)  # the whole batch on the first pipeline
    assert (p["fgrid"], p["giant_cap"], p["giant_grid"], p["small_grid"]) == (p["nbmax"], 1024, 1024, 0)


def test_stage_b_shapes(harness, tmp_path):
    assert one(harness, tmp_path, 100)["b_shape"] == B_ROWS_SPLIT
    assert one(harness, tmp_path, 100, rows=0)["b_shape"] == B_SPLIT
    assert one(harness, tmp_path, 100, big_split=0)["b_shape"] == B_ONE
    assert one(harness, tmp_path, 100, big_split=0, rows=0)["b_shape"] == B_ONE


def test_solo(harness, tmp_path):
    assert one(harness, tmp_path, 1526)["solo"] == 1
    assert one(harness, tmp_path, 1526, b_split=0)["solo"] == 0
    assert one(harness, tmp_path, 1526, v2=0)["solo"] == 0
    assert one(harness, tmp_path, 15259, no_overlap=1)["solo"] == 1           # one stream: every batch as a call of one
    assert one(harness, tmp_path, 15259)["solo"] == 0


# ---- parsing ----------------------------------------------------------------------------------------------------------------------
def _switches(harness, env, measure=False):
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("MI_LZ", "MI_LZW", "MI_LZS"))}
    r = subprocess.run([harness, "switches"], env=dict(clean, **env), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = [int(v) for v in r.stdout.split()]
    names = SW._fields if measure else SW._fields[:-3]
    assert len(vals) == len(names)
    return dict(zip(names, vals))


VALUES = [None, "", "0", "00", "1", "abc", "-1"]              # None: unset
OFF_IFF_0 = dict(zip(VALUES, [1, 1, 0, 0, 1, 1, 1]))          # off iff the first character is '0'
SET_OR_NOT = dict(zip(VALUES, [0, 1, 1, 1, 1, 1, 1]))
ATOI_ON = dict(zip(VALUES, [1, 0, 0, 0, 1, 0, 1]))            # atoi, non-zero means on; unset means on
EXPECT = {
    "v2": OFF_IFF_0, "b_split": OFF_IFF_0, "big_split": OFF_IFF_0, "sliced": OFF_IFF_0,
    "batch": dict(zip(VALUES, [0, 0, 0, 0, 1, 0, 0]), **{"4096": 4096, "4097": 0, "64": 64}),
    "rows": ATOI_ON, "prefix": ATOI_ON,
    "rows_waves": dict(zip(VALUES, [9, 0, 0, 0, 1, 0, 9]), **{"12": 12}),                  # atol; negative: the default; no clamp
    "lanes_kib": dict(zip(VALUES, [8, 1, 1, 1, 1, 1, 8]), **{"32": 32, "33": 32, "16": 16}),   # atol; negative: the default; 1..32
    "fb2_side": dict(zip(VALUES, [-1, 0, 0, 0, 1, 0, 0]), **{"10": 1}),                    # unset / first character '1' / anything else
    "no_overlap": SET_OR_NOT, "prof": SET_OR_NOT, "debug": SET_OR_NOT, "serial": SET_OR_NOT,
    # -DMI_MEASURE only
    "no_fb": SET_OR_NOT,
    "skip": dict(zip(VALUES, [0, 0, 0, 0, 1, 0, -1]), **{"3": 3}),
    "stop_phase": dict(zip(VALUES, [0, 0, 0, 0, 1, 0, 0xFFFFFFFF]), **{"5": 5}),
}


def test_defaults(harness, harness_measure):
    assert _switches(harness, {}) == {k: v for k, v in DEFAULT._asdict().items() if k not in MEASURE_ONLY}
    assert _switches(harness_measure, {}, measure=True) == DEFAULT._asdict()


@pytest.mark.parametrize("field", [f for f in SW._fields if f not in MEASURE_ONLY])
def test_parsing(harness, field):
    base = _switches(harness, {})
    for value, want in EXPECT[field].items():
        got = _switches(harness, {} if value is None else {ENV[field]: value})
        assert got == dict(base, **{field: want}), (field, value)           # and no other member moves


@pytest.mark.parametrize("field", MEASURE_ONLY)
def test_parsing_of_the_measurement_switches(harness, harness_measure, field):
    base = _switches(harness_measure, {}, measure=True)
    for value, want in EXPECT[field].items():
        env = {} if value is None else {ENV[field]: value}
        assert _switches(harness_measure, env, measure=True) == dict(base, **{field: want}), (field, value)
        assert _switches(harness, env) == _switches(harness, {})            # a shipped build does not look at them
