#!/bin/bash
# Round-3 artefacts for the current build (GPU box, repo root):  bash tools/round3_profile.sh [part ...]   parts: bench prof pmc dp fp8 big ab
# Everything goes to gpurun_out/r03/ (copy what is to be judged into profiles/r03/).
set -e
OUT=$PWD/gpurun_out/r03
mkdir -p $OUT
REPO=$PWD
PARTS=${@:-bench prof pmc dp fp8 big ab}
has() { [[ " $PARTS " == *" $1 "* ]]; }
if has bench; then
  python bench.py --full > $OUT/a_bench.json 2> $OUT/a_bench.err
  python bench.py --full --frames 1 --no-cpu-baseline > $OUT/a_bench_T1.json 2>> $OUT/a_bench.err
  echo "bench done"; head -c 300 $OUT/a_bench.json; echo
fi
if has prof; then
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o k -- python3 $REPO/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --roofline-steps 0 > $OUT/a_bench_rocprof.json 2> $OUT/a_rocprof.err
  AVSIAM_WGRAD_STREAM=0 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_s0 -o k -- python3 $REPO/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --roofline-steps 0 > $OUT/a_s0_bench_rocprof.json 2> $OUT/a_s0_rocprof.err
  cd $REPO
  find $OUT/prof -name "*kernel_stats.csv" -exec cp {} $OUT/a_kernel_stats.csv \;
  find $OUT/prof_s0 -name "*kernel_stats.csv" -exec cp {} $OUT/a_s0_kernel_stats.csv \;
  rm -rf $OUT/prof $OUT/prof_s0
  echo "prof done"; head -6 $OUT/a_s0_kernel_stats.csv
fi
if has pmc; then
  bash tools/pmc_traffic.sh r03/pmc_traffic > $OUT/pmc_traffic.log 2>&1 && cp gpurun_out/r03/pmc_traffic/traffic.json $OUT/traffic.json && cp gpurun_out/r03/pmc_traffic/traffic_by_kernel.txt $OUT/traffic_by_kernel.txt
  bash tools/pmc_busy.sh r03/pmc_busy > $OUT/pmc_busy.log 2>&1 && cp gpurun_out/r03/pmc_busy/pmc_busy.json $OUT/pmc_busy.json && cp gpurun_out/r03/pmc_busy/pmc_busy_by_kernel.txt $OUT/pmc_busy_by_kernel.txt
  echo "pmc done"; cat $OUT/pmc_busy_by_kernel.txt
fi
if has dp; then
  # the data-parallel branch on hardware at world size 1: every collective issued; torch.distributed and the C ABI's communicator,
  # fp32 and bf16 wire, overlapped chunks and one blocking message, deferred MAE-only update - against the plain line of the same box
  python bench.py --full --no-cpu-baseline --steps 10 > $OUT/dp_plain.json 2> $OUT/dp.err
  torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 1 bench.py --full --steps 10 --no-cpu-baseline --force-dp > $OUT/dp_force_torch.json 2>> $OUT/dp.err
  AVSIAM_COMM=rccl torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 1 bench.py --full --steps 10 --no-cpu-baseline --force-dp > $OUT/dp_force_rccl.json 2>> $OUT/dp.err
  AVSIAM_DP_WIRE=bf16 torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 1 bench.py --full --steps 10 --no-cpu-baseline --force-dp > $OUT/dp_force_torch_bf16wire.json 2>> $OUT/dp.err
  AVSIAM_DP_OVERLAP=0 torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 1 bench.py --full --steps 10 --no-cpu-baseline --force-dp > $OUT/dp_force_torch_blocking.json 2>> $OUT/dp.err
  AVSIAM_DP_DEFER=1 torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 1 bench.py --full --steps 10 --no-cpu-baseline --force-dp > $OUT/dp_force_torch_defer.json 2>> $OUT/dp.err
  python - <<PY
import json, glob
for f in sorted(glob.glob("$OUT/dp_*.json")):
    try:
        d = json.load(open(f)); print(f.split("/")[-1], round(d["value"], 2), round(d["ms_per_step"], 2), d["config"].get("force_dp"))
    except Exception as e:
        print(f, "ERR", e)
PY
fi
if has fp8; then
  python bench.py --full --no-cpu-baseline --steps 10 --fp8 > $OUT/b_vitb_fp8_bench.json 2> $OUT/fp8.err
  python bench.py --full --no-cpu-baseline --steps 10 --fp8 --fp8-dgrad > $OUT/b_vitb_fp8_dgrad_bench.json 2>> $OUT/fp8.err
  python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --model vit_huge14 --recompute > $OUT/h_vit_huge14_b64_recompute_bench.json 2>> $OUT/fp8.err
  python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --model vit_huge14 --recompute --fp8 > $OUT/h_vit_huge14_b64_recompute_fp8_bench.json 2>> $OUT/fp8.err
  python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --model vit_huge14 --recompute --fp8 --fp8-dgrad > $OUT/h_vit_huge14_b64_recompute_fp8_dgrad_bench.json 2>> $OUT/fp8.err
  python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --model vit_huge14 --recompute 0.375 > $OUT/h_vit_huge14_b64_recompute0375_bench.json 2>> $OUT/fp8.err
  python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --model vit_huge14 --recompute 0.375 --fp8 --fp8-dgrad > $OUT/h_vit_huge14_b64_recompute0375_fp8_dgrad_bench.json 2>> $OUT/fp8.err
  python - <<PY
import json, glob
for f in sorted(glob.glob("$OUT/[bh]_*bench.json")):
    try:
        d = json.load(open(f)); print(f.split("/")[-1], round(d["value"], 2), round(d["ms_per_step"], 2), "bf16 frac", round(d["roofline"]["frac"], 3), "fp8 frac", d.get("roofline_fp8", {}).get("frac"))
    except Exception as e:
        print(f, "ERR", e)
PY
fi
if has big; then
  python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --model vit_large > $OUT/l_vit_large_bench.json 2> $OUT/big.err
  python -c "import json; d=json.load(open('$OUT/l_vit_large_bench.json')); print('vit_large', d['value'], d['ms_per_step'], d['roofline']['frac'])"
fi
if has ab; then
  # the round-2 build (ab_r02/: the tree at the round-2 commit with its own library) against this one on THIS box, alternating
  for v in r02 r03 r02 r03; do
    if [ $v = r02 ]; then (cd ab_r02 && python bench.py --no-cpu-baseline --steps 10 2>/dev/null) > $OUT/ab_${v}_$RANDOM.json; else python bench.py --full --no-cpu-baseline --steps 10 2>/dev/null > $OUT/ab_${v}_$RANDOM.json; fi
  done
  python - <<PY
import json, glob
for f in sorted(glob.glob("$OUT/ab_r0*.json")):
    d = json.load(open(f)); print(f.split("/")[-1], round(d["value"], 2), round(d["ms_per_step"], 2), round(d["roofline"]["frac"], 4))
PY
fi
