tag=$1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${O:-prof_out}; mkdir -p $O  # where the logs and digests go
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/pc2 -- python3 bench.py --steps 40 --warmup 5 --no-overlap --no-cpu-baseline --timed-only > $O/${tag}_prof_serial.log 2>&1 || exit 1
python3 tools/chain_timeline.py $O/pc2 20 > $O/${tag}_timeline_serial.txt 2>&1; rm -rf $O/pc2
cat $O/${tag}_timeline_serial.txt
for wl in twitter uk-2006-05; do
  timeout -k 10 500 python3 bench.py --full --workload $wl --steps 60 > $O/${tag}_bench_$wl.json 2> $O/${tag}_bench_$wl.err; echo "$wl rc=$?"
  python3 tools/show_bench.py $O/${tag}_bench_$wl.json | grep -E '"value"|ms_per_step|frac|edges_per_s|edges_per_step|input_nodes' | head -12
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/pc3 -- python3 bench.py --workload $wl --steps 20 --warmup 3 --no-overlap --no-cpu-baseline --timed-only > $O/${tag}_prof_serial_$wl.log 2>&1 || exit 1
  cp $(find $O/pc3 -name "*kernel_stats.csv") $O/${tag}_bench_${wl}_serial_kernel_stats.csv
  python3 tools/chain_timeline.py $O/pc3 10 > $O/${tag}_timeline_serial_$wl.txt 2>&1; rm -rf $O/pc3
  tail -3 $O/${tag}_timeline_serial_$wl.txt
done
for st in khop0 khop1 weighted_khop weighted_khop_hash_dedup; do
  timeout -k 10 400 python3 bench.py --no-cpu-baseline --no-extract-leg --no-train-leg --sample-type $st > $O/ab_tmp.json 2> $O/ab_tmp.err
  echo "$st $(python3 tools/show_bench.py $O/ab_tmp.json | grep -E '\"value\"|\"ms_per_step\"|edges_per_step' | head -3 | tr -d '\n')"
done | tee $O/${tag}_sample_types.txt
