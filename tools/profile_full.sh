# usage: bash tools/profile_full.sh <tag> [pytest|nopytest]  -- GPU box: whole GPU suite, default bench, rocprof stats + serial
# timeline of the same command, PMC passes (separate), then the 1S+1T pipeline with both ranks on the one GPU
tag=$1; what=${2:-pytest}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${O:-prof_out}; mkdir -p $O  # where the logs and digests go
if [ "$what" = pytest ]; then
  timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $O/${tag}_pytest.log 2>&1; rc=$?
  echo "pytest rc=$rc"; tail -5 $O/${tag}_pytest.log
  [ $rc -ne 0 ] && exit $rc
fi
timeout -k 10 500 python3 bench.py --full > $O/${tag}_bench_default.json 2> $O/${tag}_bench_default.err; rc=$?
echo "bench rc=$rc"; [ $rc -ne 0 ] && { tail -c 2000 $O/${tag}_bench_default.err; exit $rc; }
python3 tools/show_bench.py $O/${tag}_bench_default.json | grep -E '"value"|ms_per_step|frac|edges_per_s|hit_rate|GBps' | head -40
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/pc1 -- python3 bench.py --no-cpu-baseline --timed-only > $O/${tag}_prof_default.log 2>&1 || exit 1
python3 tools/stats_summary.py $O/pc1 > $O/${tag}_default_stats.md
cp $(find $O/pc1 -name "*kernel_stats.csv") $O/${tag}_bench_default_kernel_stats.csv
python3 tools/overlap_stats.py $O/pc1 > $O/${tag}_overlap.txt 2>&1
rm -rf $O/pc1
head -25 $O/${tag}_default_stats.md
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/pc2 -- python3 bench.py --steps 40 --warmup 5 --no-overlap --no-cpu-baseline --timed-only > $O/${tag}_prof_serial.log 2>&1 || exit 1
python3 tools/chain_timeline.py $O/pc2 20 > $O/${tag}_timeline_serial.txt 2>&1; rm -rf $O/pc2
cat $O/${tag}_timeline_serial.txt
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_$c -- python3 bench.py --steps 20 --warmup 3 --no-overlap --no-cpu-baseline --timed-only > $O/${tag}_pmc_$c.log 2>&1 || exit 1
done
python3 tools/pmc_summary.py $O/pmc_FETCH_SIZE $O/pmc_WRITE_SIZE $O/${tag}_pmc_FETCH_SIZE.log > $O/${tag}_pmc_traffic.json 2> $O/${tag}_pmc.err
rm -rf $O/pmc_FETCH_SIZE $O/pmc_WRITE_SIZE
head -12 $O/${tag}_pmc_traffic.json; tail -3 $O/${tag}_pmc.err
# config 3's trainer-side leg from KERNEL durations: (a) bench.py's roofline_extract (this GPU samples too), (b) the
# trainer process of the decoupled 1S+1T run (the trainer drains a full queue alone); rocprofv3's preloaded library is
# inherited by the rank processes bench.py starts, one trace per process
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/px1 -- python3 bench.py --full --steps 64 --warmup 5 --windows 1 --no-train-leg --no-cpu-baseline --presample-variants "" > $O/${tag}_prof_extract_leg.log 2>&1 || exit 1
python3 - <<P > $O/${tag}_extract_kernel_stats.md
import json, subprocess
l = json.loads([x for x in open("$O/${tag}_prof_extract_leg.log") if x.startswith("{")][-1])
r = l["roofline_extract"]
print("## roofline_extract under rocprofv3 --kernel-trace (presample_epoch %d, hit rate %.4f, %.4f ms per batch in this profiled run)" % (r["presample_epoch"], r["hit_rate"], r["ms_per_step"]))
print(subprocess.run(["python3", "tools/extract_kernel_rates.py", "$O/px1", str(r["miss"]["bytes_per_step"]), str(r["cached"]["bytes_per_step"])], capture_output=True, text=True).stdout)
P
python3 tools/stats_summary.py $O/px1 >> $O/${tag}_extract_kernel_stats.md; rm -rf $O/px1
timeout -k 10 500 rocprofv3 --kernel-trace --output-format csv -d $O/px2 -- python3 bench.py --gpus 2 --decoupled --no-train-leg --no-cpu-baseline > $O/${tag}_prof_decoupled.log 2>&1 || exit 1
python3 - <<P >> $O/${tag}_extract_kernel_stats.md
import json, subprocess
l = json.loads([x for x in open("$O/${tag}_prof_decoupled.log") if x.startswith("{")][-1])
pl = l["pipeline"]
rows = l["input_nodes_per_step"]; miss_b = pl["miss"]["bytes_per_step"]; hit_b = (rows - miss_b / 512.0) * (2 * 512 + 8)
print("\n## the trainer PROCESS of bench.py --gpus 2 --decoupled under rocprofv3 --kernel-trace (it drains a full queue alone; %.4f ms per batch, second half %.4f)" % (l["ms_per_step"], pl["consumed_second_half_ms_per_batch"]))
print(subprocess.run(["python3", "tools/extract_kernel_rates.py", "$O/px2", str(miss_b), str(hit_b)], capture_output=True, text=True).stdout)
P
rm -rf $O/px2; cat $O/${tag}_extract_kernel_stats.md
timeout -k 10 500 python3 bench.py --gpus 2 --full --no-cpu-baseline > $O/${tag}_bench_gpus2.json 2> $O/${tag}_bench_gpus2.err; echo "bench2 rc=$?"
tail -c 800 $O/${tag}_bench_gpus2.err
python3 tools/show_bench.py $O/${tag}_bench_gpus2.json | head -60
