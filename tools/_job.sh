set -o pipefail
out=${1:?usage: bash tools/_job.sh <output directory>}
mkdir -p "$out"
timeout -k 10 1100 python3 -m pytest tests -x -q -m gpu > "$out"/pytest_gpu.log 2>&1; rc=$?; echo "pytest rc $rc"; tail -3 "$out"/pytest_gpu.log
[ $rc -eq 0 ] || exit 1
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out"/smoke.txt 2>&1; tail -1 "$out"/smoke.txt
python3 bench.py --full > "$out"/bench_default.json 2>"$out"/e1.txt || exit 1
python3 bench.py --workload sites > "$out"/bench_cfg4.json 2>"$out"/e2.txt || exit 1
python3 bench.py --workload network > "$out"/bench_cfg5_joingraph.json 2>"$out"/e3.txt || exit 1
python3 bench.py --workload network --graph bethe > "$out"/bench_cfg5_bethe.json 2>"$out"/e4.txt || exit 1
PGBP_BENCH_REHEARSAL=1 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29655 bench.py --gpus 2 --steps 5 --warmup 2 --full --no-cpu-baseline > "$out"/bench_default_2rank_rehearsal_one_gpu.json 2>"$out"/e5.txt; echo "rehearsal rc $?"
tail -c 200 "$out"/bench_default_2rank_rehearsal_one_gpu.json
