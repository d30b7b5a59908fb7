#!/bin/bash
# Issue counters of gemm_nt_q8_kernel at the two stage-2 Mlp shapes (counters only, a run of its own per shape; style of tools/pmc_tn_lds.sh).
#   tools/pmc_q8_loop.sh <tag> [library]      -> $FIBER_PMC_OUT (default build/pmc) /pmc_q8_<tag>_<shape>/, one summary line per shape on stdout
# Units: SQ counters are summed over waves (SQ_WAVE_CYCLES, SQ_WAIT_ANY, SQ_ACTIVE_INST_ANY in quad-cycles).
cd "$(dirname "$0")/.." || exit 1
TAG=${1:-tree}
[ -n "$2" ] && export FIBER_HIP_LIB=$(realpath "$2")
export TMPDIR=/tmp
OUT=${FIBER_PMC_OUT:-build/pmc}
mkdir -p $OUT
for shp in "294912 1536 512" "294912 512 2048"; do
  d=$OUT/pmc_q8_${TAG}_$(echo $shp | tr ' ' x)
  timeout -k 10 240 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_SALU SQ_INSTS_VALU -d $d --output-format csv -- \
    python tools/probes/pmc_q8.py $shp > $d.log 2>&1 || { echo "pass $TAG $shp failed: rc=$?"; tail -5 $d.log; exit 1; }
  f=$(find $d -name "*counter_collection.csv" | head -1)
  python - "$f" "$TAG" "$shp" <<'PY'
import collections, csv, sys
acc = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    if "gemm_nt_q8_kernel" in r["Kernel_Name"]:
        acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
print(sys.argv[2], "[" + sys.argv[3].replace(" ", ", ") + "]", {c: round(sum(v) / len(v)) for c, v in sorted(acc.items())}, "launches", {len(v) for v in acc.values()})
PY
done
