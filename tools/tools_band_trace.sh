#!/bin/bash
# kernel trace of one band of an N-way split: bash tools_band_trace.sh <tag> <workload> <N> [local|rccl] [more tools_band_time.py arguments]
# (e.g. ... c4 8 local --tracers 4 --tracer-scheme van_leer --tracer-rows 2: the tracer launches are then summarised by grid size --
#  the small grid is the edge-row launch, which sits on the exchange chain ahead of the pack)
TAG=$1; WL=$2; N=$3; EX=${4:-local}; shift $(( $# < 4 ? $# : 4 ))
BAND_TIME=$(cd "$(dirname "$0")" && pwd)/tools_band_time.py
OUT=/root/repo/gpurun_out/bandtrace_$TAG
rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -- python3 $BAND_TIME --workload $WL --splits $N --steps 10 --exchange $EX "$@" > $OUT/out.txt 2> $OUT/err.txt
python3 - <<PY
import csv, glob
f = glob.glob("$OUT/*/*_kernel_trace.csv")[0]
rows = [r for r in csv.DictReader(open(f))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
k = [i for i, r in enumerate(rows) if "spu_filter" in r["Kernel_Name"] or "fused" in r["Kernel_Name"]]
i0 = k[len(k) // 2]
t0 = int(rows[i0]["Start_Timestamp"])
tr = {}
for r in rows[len(rows) // 2:]:
    if "pe_tracer" in r["Kernel_Name"]:
        key = (r["Kernel_Name"].replace("void gcm::", "").split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size")))
        tr.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (name, grid), d in sorted(tr.items()):
    d.sort()
    print("tracer launch %-52s grid %6s  n %4d  median %7.1f us  min %7.1f  max %7.1f" % (name, grid, len(d), d[len(d) // 2], d[0], d[-1]))
for r in rows[i0:i0 + 30]:
    print("%-34s q=%s start %8.1f end %8.1f dur %7.1f us grid %s" % (r["Kernel_Name"].replace("void gcm::", "")[:34], r.get("Queue_Id"), (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r.get("Grid_Size_X", r.get("Grid_Size"))))
PY
