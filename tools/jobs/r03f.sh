# Round-3 evidence on the final build: GPU suite, bench lines, two-column kernel table, rocprof kernel stats of bench
# (with and without the fresh-input leg), group fan-out.
set -e
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r03f; mkdir -p $O
cd $R
python -m pytest tests -x -q -m gpu --durations=6 > $O/pytest_gpu.log 2>&1 || { tail -60 $O/pytest_gpu.log; exit 1; }
tail -10 $O/pytest_gpu.log
python bench.py --full > $O/bench_n1.json 2> $O/bench_n1.err
python bench.py --full --steps 20 --warmup 5 > $O/bench_n1_driver_flags.json 2>> $O/bench_n1.err
rm -f $O/bench_all_workloads.jsonl
for w in "--rows 2048" "--rows 2048 --graph" "--workload masked_chain" "--workload masked_chain --fused" "--workload minmax" "--workload minmax --side 32768" "--workload minmax --side 65536 --steps 20 --warmup 3" "--workload ndvi" "--workload ndvi --fused" "--workload ndvi --mixed" "--workload ndvi --fused --mixed" "--workload binop --lt u16 --rt u16 --op add" "--workload binop --lt f32 --rt f32 --op add" "--workload binop --lt u8 --rt u8 --op add" "--side 32768 --steps 40"; do
  python bench.py --full $w --no-cpu-baseline >> $O/bench_all_workloads.jsonl 2>> $O/bench_all.err
done
python tools/kernel_table.py > $O/kernel_table.md 2> $O/kernel_table.err || { tail -20 $O/kernel_table.err; exit 1; }
echo "| G | cells/shard | K | async host/wall/gpu us | blocking host/wall/gpu us | plain one thread host/wall/gpu us | async again |" > $O/group_fanout_rows.md
for G in 1 2 4 8; do
  timeout -k 10 120 ./tools/group_bench $G 65536 400 >> $O/group_fanout_rows.md 2>> $O/group_bench.err
  timeout -k 10 120 ./tools/group_bench $G $((33554432 / G)) 400 >> $O/group_fanout_rows.md 2>> $O/group_bench.err
done
cat $O/group_fanout_rows.md
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_bench --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline > $O/bench_under_rocprof.json 2> $O/prof_bench.err
rocprofv3 --kernel-trace --stats -d $O/prof_bench_loop --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --no-fresh-inputs --no-reference-streams > $O/bench_loop_only_under_rocprof.json 2> $O/prof_bench_loop.err
rocprofv3 --kernel-trace --stats -d $O/prof_table --output-format csv -- python3 /root/repo/tools/kernel_table.py > $O/kernel_table_under_rocprof.md 2> $O/prof_table.err
cd $R
for d in prof_bench prof_bench_loop prof_table; do
  f=$(find $O/$d -name '*kernel_stats.csv' | head -1); [ -n "$f" ] && cp $f $O/${d}_kernel_stats.csv
  find $O/$d -name '*.csv' -size +1M -delete
done
head -4 $O/prof_bench_loop_kernel_stats.csv | cut -c1-260
python - <<'PY'
import json
for f in ("bench_n1.json", "bench_n1_driver_flags.json", "bench_under_rocprof.json", "bench_loop_only_under_rocprof.json"):
    r = json.load(open("gpurun_out/r03f/" + f)); rf = r["roofline"]
    print(f, round(r["value"], 1), round(rf["frac"], 4), round(rf["launch_ms"], 5), rf.get("fresh_inputs", {}).get("frac"))
for l in open("gpurun_out/r03f/bench_all_workloads.jsonl"):
    r = json.loads(l)
    print(f"{r['config']['workload'][:78]:78s} {r['value']:8.1f} Gcells/s  frac {r['roofline']['frac']:.3f}")
PY
