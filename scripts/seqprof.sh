ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d); cd $TMP; export TMPDIR=$TMP
python -m pytest $ROOT/tests/test_gpu_fused_learner.py $ROOT/tests/test_gpu_trainer.py -x -q -m gpu -k "meta or golden or data_parallel or two_ranks" 2>&1 | tail -2
rocprofv3 --kernel-trace --stats -d $TMP/tr -o t -- python $ROOT/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline > $TMP/b.json 2>/dev/null
python $ROOT/scripts/top_kernels.py $TMP/tr/t_results.db 8 | head -12
tail -1 $TMP/b.json | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['phases']['meta_ms'])"
python $ROOT/bench.py --full --no-cpu-baseline 2>/dev/null | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['phases']['meta_ms'])"
