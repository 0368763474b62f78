cd /tmp && export TMPDIR=/tmp
export GPU_MAX_HW_QUEUES=8   # the setting bench.py gives itself; under rocprofv3 the runtime is up before Python runs
cd $GRAFT_REPO_ROOT
O=${1:?usage: tools/run_prof.sh OUT_DIR}
mkdir -p $O
python bench.py --full --steps 200 --warmup 10 > $O/bench_default.json 2> $O/bench_default.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_shared -- python3 bench.py --regime shared --steps 50 --warmup 5 --cpu-sample 0 > $O/bench_shared_prof.json 2> $O/bench_shared_prof.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_indep -- python3 bench.py --steps 50 --warmup 5 --cpu-sample 0 > $O/bench_indep_prof.json 2> $O/bench_indep_prof.err
ls -R $O/prof_shared | head
tail -c 600 $O/bench_default.json
python bench.py --chunks 2 --cpu-sample 0 > $O/bench_chunks2.json 2>/dev/null
python bench.py --dtype f64 --cpu-sample 0 > $O/bench_f64.json 2>/dev/null
