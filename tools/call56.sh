cd $GRAFT_REPO_ROOT; mkdir -p gpurun_out/c56; O=$GRAFT_REPO_ROOT/gpurun_out/c56
bash tools/ab.sh "MN_X=0" "HSA_ENABLE_INTERRUPT=0" "ROC_ACTIVE_WAIT_TIMEOUT=100" 2>&1 | tee $O/ab.txt
