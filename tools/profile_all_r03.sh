cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
bash tools/profile_r03.sh r03_v7 > $OUT/r3_prof_v7_c3.log 2>&1
bash tools/profile_r03.sh r03_v7_c2 cornell 512 512 64 0 > $OUT/r3_prof_v7_c2.log 2>&1
bash tools/profile_r03.sh r03_v7_c4 teapot 1920 1080 256 200000 > $OUT/r3_prof_v7_c4.log 2>&1
tail -11 $OUT/r3_prof_v7_c3.log
tail -4 $OUT/r3_prof_v7_c2.log
tail -4 $OUT/r3_prof_v7_c4.log
timeout -k 5 300 python tools/stripe_probe.py 1 2 4 8 > $OUT/r3_stripe.log 2>&1; cat $OUT/r3_stripe.log | grep -v amdgpu
timeout -k 5 600 python bench.py --full > $OUT/r3_bench_full.json 2> $OUT/r3_bench_full.err; tail -c 600 $OUT/r3_bench_full.json
