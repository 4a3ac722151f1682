#!/bin/bash
# Memory-path counters of the five dense 3 x 3 launches of a step for one library build and dispatch mode, per launch:
#   tools/pmc_conv_halo.sh TAG MODE [lib.so]   (MODE: ocv_conv3x3_set_dispatch, 1 = tap ring, 2 = halo-staged, 0 = automatic)
# rocprofv3 --pmc in a run of its own (no tracing) over tools/conv_halo_ab.py; output under ${OUT:-runs}/pmc_conv_halo/TAG.
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
tag=$1; mode=$2; d=${OUT:-runs}/pmc_conv_halo/$tag; rm -rf $d; mkdir -p $d
[ -n "$3" ] && export OCV_LIB_PATH=$3
rocprofv3 --pmc TCP_TCC_READ_REQ_sum SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD --output-format csv -d $d/a -- python3 tools/conv_halo_ab.py $mode > $d/a.log 2>&1 || { tail -3 $d/a.log; exit 1; }
python3 - $d <<'PY'
import collections, csv, glob, sys
d = sys.argv[1]
f = glob.glob(d + "/a/*/*_counter_collection.csv")[0]
per = collections.defaultdict(lambda: collections.defaultdict(float))
cnt = collections.defaultdict(lambda: collections.defaultdict(int))
for r in csv.DictReader(open(f)):
    k = r["Kernel_Name"]
    if "conv_split_dma_kernel" in k or "conv_halo_dma_kernel" in k:
        key = (k[k.index("conv_"):].split("(")[0], int(r["Grid_Size"]) // max(int(r["Workgroup_Size"]), 1))
        per[key][r["Counter_Name"]] += float(r["Counter_Value"])
        cnt[key][r["Counter_Name"]] += 1
for key, m in sorted(per.items()):
    print(f"{d} {key[0]} [wgs={key[1]}]: " + "  ".join(f"{c} {m[c] / cnt[key][c]:.0f} (n={cnt[key][c]})" for c in sorted(m)))
PY
