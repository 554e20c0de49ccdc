# Round-5 profiles: the rocprofv3 kernel trace + stats of the EXACT driver command
# (python3 bench.py --gpus 1 --steps 20 --warmup 5) and PMC passes (each its own run, within the
# per-block counter limits) of a short headline-only bench run; the FASTQ flow breakdown.
# Output under gpurun_out/prof5h/; tools/summarize_profile.py --round r05 --src gpurun_out/prof5h.
set -u
cd "$GRAFT_REPO_ROOT"
P=gpurun_out/prof5h
mkdir -p $P
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $P/trace -o run --output-format csv -- \
  python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $P/trace.log 2>&1 || exit 3
B="python3 bench.py --full --no-cpu --no-paths --pair-steps 0 --steps 5 --warmup 2"
i=0
for pmc in "SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE GRBM_COUNT" \
           "FETCH_SIZE" "WRITE_SIZE" \
           "SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT SQ_BUSY_CYCLES SQ_ACTIVE_INST_LDS SQ_VALU_MFMA_COEXEC_CYCLES TCC_HIT_sum TCC_MISS_sum"; do
  i=$((i+1))
  timeout -s KILL 120 rocprofv3 --pmc $pmc -d $P/pmc$i -o run --output-format csv -- $B > $P/pmc$i.log 2>&1 || echo "pmc pass $i failed"
done
timeout -k 10 300 python3 tools/fastq_flow_breakdown.py > $P/fastq_flow.json 2> $P/fastq_flow.err || exit 3
echo done
