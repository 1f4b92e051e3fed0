#!/bin/bash
# per-phase instruction counts of k_lz2_find: the kernel leaves after phase k (MI_LZ_STOP_PHASE=k, measurement only — the
# output of such a run is wrong by construction), one counter pass per k; differences between successive k are the phases.
# A last pass (k = 0, a run of its own) takes SQ_BUSY_CYCLES.  The whole-kernel rows of k_lz2_partition come from the k = 0 passes.
# Needs a MEASUREMENT build of the library (the shipped one ignores MI_LZ_STOP_PHASE):
#   make -C compression_algorithms_amd/csrc OUT=../lib_measure EXTRA=-DMI_MEASURE     (in the build container, before gpurun)
#   PHASE_PMC_LIB     directory under compression_algorithms_amd/ that holds it (lib_measure)
#   PHASE_PMC_TAG     suffix of the output directory, $OUT below: phase_pmc_TAG (none)
#   PHASE_PMC_PHASES  the passes to run ("1 2 3 4 5 6 7 0"; "1 0" gives phase "gather" against the whole kernel)
#   PHASE_PMC_TIMEOUT seconds every pass may take (300)
# Every pass runs under its own time limit, and the first pass that fails ends the script: nothing more is started on a GPU
# that a pass has just faulted or hung.
OUT=gpurun_out/phase_pmc; mkdir -p $OUT; export TMPDIR=/tmp
set -u
LIBDIR=${PHASE_PMC_LIB:-lib_measure}
if [ -n "${PHASE_PMC_TAG:-}" ]; then rmdir $OUT 2> /dev/null; OUT=${OUT}_$PHASE_PMC_TAG; mkdir -p "$OUT"; fi
PHASES=${PHASE_PMC_PHASES:-1 2 3 4 5 6 7 0}
LIMIT=${PHASE_PMC_TIMEOUT:-300}
export MI_CODEC_LIB=$PWD/compression_algorithms_amd/$LIBDIR/libmi_codec.so
[ -f "$MI_CODEC_LIB" ] || { echo "build $LIBDIR first (see the header of this script)"; exit 1; }
cat > "$OUT/drv.py" <<'PY'
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from compression_algorithms_amd import lz, synth
from compression_algorithms_amd.context import Context
ctx = Context(0)
x = synth.enwik_like(67108864, seed=12345, device="cuda")
lz.compress(x, lz.params("deflate"), ctx)
torch.cuda.synchronize()
PY
export MI_LZ_NO_OVERLAP=1
for k in $PHASES; do
  MI_LZ_STOP_PHASE=$k timeout -k 10 "$LIMIT" rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU \
      --output-format csv -d "$OUT/k$k" -- python3 "$OUT/drv.py" > "$OUT/k$k.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass k=$k failed (exit status $rc): stopping"; tail -3 "$OUT/k$k.log"; exit $rc; fi
done
MI_LZ_STOP_PHASE=0 timeout -k 10 "$LIMIT" rocprofv3 --pmc SQ_BUSY_CYCLES SQ_WAVES --output-format csv -d "$OUT/busy" -- python3 "$OUT/drv.py" > "$OUT/busy.log" 2>&1
rc=$?
if [ $rc -ne 0 ]; then echo "pass SQ_BUSY_CYCLES failed (exit status $rc): stopping"; tail -3 "$OUT/busy.log"; exit $rc; fi
python3 - "$OUT" $PHASES <<'PY' | tee "$OUT/summary.txt"
import csv, glob, sys
from collections import defaultdict
out, phases = sys.argv[1], [int(v) for v in sys.argv[2:]]
names = ["gather", "sort_home", "sweep", "sort_cluster", "permute", "lane_replay", "export+out"]
COLS = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU")


def collect(d, name):
    acc = defaultdict(float)
    for f in glob.glob(f"{out}/{d}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if name in r["Kernel_Name"]:
                acc[r["Counter_Name"]] += float(r["Counter_Value"])
    return acc


def line(label, cur, prev):
    return (f"{label:14s} " + " ".join(f"{(cur[c] - prev[c]) / 1e6:12.1f}" for c in COLS[:3]) + " " +
            " ".join(f"{(cur[c] - prev[c]) / 1e6:10.2f}" for c in COLS[3:5]) +
            f" {(cur['SQ_WAVE_CYCLES'] - prev['SQ_WAVE_CYCLES']) / 1e6:14.1f} {(cur['SQ_ACTIVE_INST_VALU'] - prev['SQ_ACTIVE_INST_VALU']) / 1e6:12.1f}")


rows = {k: collect(f"k{k}", "k_lz2_find") for k in phases}
zero = defaultdict(float)
print(f"{'phase':14s} {'VALU':>12s} {'SALU':>12s} {'LDS':>12s} {'VMEM_RD':>10s} {'VMEM_WR':>10s} {'WAVE_CYC':>14s} {'ACT_VALU':>12s}   (millions per launch of 1024 blocks, differences of cumulative passes)")
prev = zero
for k in sorted(k for k in phases if k):
    print(line(names[k - 1], rows[k], prev) + ("" if k == 1 or (k - 1) in phases else f"   (everything since pass {max([0] + [j for j in phases if 0 < j < k])})"))
    prev = rows[k]
if 0 in phases:
    full = rows[0]
    print(line("full kernel", full, zero))
    if full["SQ_WAVE_CYCLES"]:
        print(f"k_lz2_find: SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES = {full['SQ_ACTIVE_INST_VALU'] / full['SQ_WAVE_CYCLES']:.4f} of a wave's life issuing VALU; "
              f"x 8 resident waves per SIMD (four workgroups of 512 per CU) = {8 * full['SQ_ACTIVE_INST_VALU'] / full['SQ_WAVE_CYCLES']:.3f} of the VALU pipe")
        if 1 in phases and full["SQ_INSTS_VALU"]:
            print(f"k_lz2_find: share of SQ_INSTS_VALU before LZ2_TICK(0) (phase gather) = {rows[1]['SQ_INSTS_VALU'] / full['SQ_INSTS_VALU']:.4f}")
    part = collect("k0", "k_lz2_partition")
    if part:
        print(line("k_lz2_partition", part, zero))
        if part["SQ_WAVE_CYCLES"]:
            print(f"k_lz2_partition: SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES = {part['SQ_ACTIVE_INST_VALU'] / part['SQ_WAVE_CYCLES']:.4f}; x 4 resident waves per SIMD (one workgroup of 1024 per CU) = "
                  f"{4 * part['SQ_ACTIVE_INST_VALU'] / part['SQ_WAVE_CYCLES']:.3f} of the VALU pipe")
for f in glob.glob(f"{out}/busy/**/*counter_collection.csv", recursive=True):
    acc = defaultdict(float)
    for r in csv.DictReader(open(f)):
        if "k_lz2_find" in r["Kernel_Name"] or "k_lz2_partition" in r["Kernel_Name"]:
            acc[(r["Kernel_Name"][:60], r["Counter_Name"])] += float(r["Counter_Value"])
    for (kn, cn), v in sorted(acc.items()):
        print(f"{cn:16s} {v / 1e6:12.2f} M  {kn}")
PY
