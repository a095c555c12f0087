set -u
# the bench / profile set of a round; every result goes under OUT_DIR
out=${1:?usage: bash tools/final_run.sh OUT_DIR}
cd $GRAFT_REPO_ROOT
mkdir -p "$out"
timeout 600 python -m pytest tests -m gpu -x -q > $out/pytest.log 2>&1; grep -E "passed|failed|error" $out/pytest.log | tail -2
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 | cut -c1-200
timeout 400 python bench.py --full > $out/bench.json 2> $out/bench.err; tail -c 400 $out/bench.json | head -c 10 >/dev/null
timeout 400 python bench.py --gpus 1 --steps 20 --warmup 5 > $out/bench_driver.json 2>> $out/bench.err
timeout 300 python bench.py --full --atoms 250000 --no-other-configs > $out/bench_250k.json 2>> $out/bench.err
timeout 300 python bench.py --full --atoms 1000000 --steps 100 --no-other-configs > $out/bench_1m.json 2>> $out/bench.err
timeout 300 python bench.py --full --workload standin --no-other-configs > $out/standin_bench.json 2>> $out/bench.err
timeout 300 python bench.py --full --workload standin --batch 64 --no-other-configs > $out/batch64_bench.json 2>> $out/bench.err
timeout 300 python bench.py --full --workload standin --batch 8 --no-other-configs > $out/batch8_bench.json 2>> $out/bench.err
timeout 300 python tools/rings_bench.py > $out/rings_bench.json 2>> $out/bench.err
timeout 300 python tools/small_bench.py --n-res 8000 > $out/chain_bench.json 2>> $out/bench.err
for k in 1 2 3; do python tools/first_pass_probe.py --tag final --e2e; done > $out/first_pass.jsonl 2>> $out/bench.err
python tools/first_pass_probe.py --tag final_standin --workload standin --e2e >> $out/first_pass.jsonl 2>> $out/bench.err
bash tools/profile.sh r6a > $out/profile.log 2>&1
bash tools/profile.sh r6a_1m "--atoms 1000000 --steps 10" > $out/profile_1m.log 2>&1
bash tools/profile.sh r6a_250k "--atoms 250000 --steps 20" > $out/profile_250k.log 2>&1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $out/fresh; timeout 200 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d $out/fresh -o t -- python tools/fresh_probe.py e2e > $out/fresh/log 2>&1
python tools/fresh_timeline.py $(find $out/fresh -name "t_kernel_trace.csv") $(find $out/fresh -name "t_memory_copy_trace.csv") > $out/e2e_timeline.txt
for f in $out/*bench*.json; do echo "$f: $(tail -1 $f | cut -c1-160)"; done
cat $out/first_pass.jsonl | cut -c1-200
tail -5 $out/bench.err
