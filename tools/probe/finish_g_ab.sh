# the finish launch with its default workgroups per query against one per query (LB_FINISH_G=1), diagnostic build
export LB_GPU_SO=$PWD/longbow_amd/liblongbow_gpu_diag.so
echo "== default"; SWEEP=1,32,64,128 python3 tools/bench_sweep.py 2>&1 | grep "B="
echo "== G=1 at 32"; LB_FINISH_G=1 SWEEP=32 python3 tools/bench_sweep.py 2>&1 | grep "B="
