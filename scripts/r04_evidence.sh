#!/usr/bin/env bash
# round 4 evidence (one GPU visit): suite, the driver-style bench line, rocprofv3 kernel trace of the bench (summary with
# the warm-up launches discarded: VERDICT r03 weak 10), the two PMC passes for k_stats, and the per-command evidence.
TAG=${1:-r04g}
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=$(pwd); O=$R/gpurun_out; mkdir -p $O; cd $R
(timeout 1500 python -m pytest tests -m gpu -q -x -n 4 2>&1 | tail -5) > $O/tests_$TAG.log 2>&1
(timeout 900 python bench.py --full 2>$O/bench_$TAG.err | tail -1) > $O/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o stats -- python $R/bench.py --full --steps 12 --warmup 3 --no-cpu-baseline --no-ops) > $O/prof_$TAG.log 2>&1
(timeout 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_$TAG -o pmc -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-ops) > $O/pmc_fetch_$TAG.log 2>&1
(timeout 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write_$TAG -o pmc -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-ops) > $O/pmc_write_$TAG.log 2>&1
cd $R
python - <<PY
import csv, glob, json, statistics
f = glob.glob("$O/prof_$TAG/**/stats_kernel_trace.csv", recursive=True)[0]
by = {}
for r in csv.DictReader(open(f)):
    by.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
out = {"source": "rocprofv3 --kernel-trace of (python bench.py --full --steps 12 --warmup 3 --no-cpu-baseline --no-ops); per kernel the launches in "
                 "time order with the first 3 (warm-up, cold caches / clocks) DISCARDED: mean / median / min / max of the rest, ms", "kernels": {}}
for k, v in by.items():
    if "k_stats" not in k and "k_prep" not in k:
        continue
    v.sort()
    d = [x[1] / 1e6 for x in v][3:] or [x[1] / 1e6 for x in v]
    out["kernels"][k[:90]] = {"launches": len(v), "kept": len(d), "mean_ms": round(statistics.mean(d), 4), "median_ms": round(statistics.median(d), 4),
                              "min_ms": round(min(d), 4), "max_ms": round(max(d), 4)}
json.dump(out, open("$O/kernel_stats_trimmed_$TAG.json", "w"), indent=1)
print(json.dumps(out["kernels"], indent=1))
PY
cat $O/tests_$TAG.log; head -c 700 $O/bench_$TAG.json; echo
bash scripts/ops_evidence.sh $TAG seq,subseq,grep,locate,rmdup,translate > $O/ops_evidence_$TAG.log 2>&1; tail -5 $O/ops_evidence_$TAG.log
