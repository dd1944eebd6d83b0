#!/bin/bash
# diagnostics: SQ counters of the count pipeline kernels on the count-only bench workload
export TMPDIR=/tmp; R=$GRAFT_REPO_ROOT; cd /tmp
export OUT=${OUT:-$R/scripts_out}; mkdir -p $OUT  # what the runs write
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_WR"; do
  i=$((i+1))
  timeout -k 10 200 rocprofv3 --pmc $set --output-format csv -d $OUT/pmc_ct_$i -- python3 $R/bench.py --full --workload ont_k31_count --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_ct_$i.log 2>&1 || echo "pass $i failed"
done
python3 - <<'PY'
import csv,glob,os,collections
R=os.environ["GRAFT_REPO_ROOT"]
acc=collections.defaultdict(lambda: collections.defaultdict(float))
for f in sorted(glob.glob(os.environ["OUT"]+"/pmc_ct_*/*/*_counter_collection.csv")):
    for r in csv.DictReader(open(f)):
        n=r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ","").replace("kmu::","").strip()
        if n.startswith("k_part") or n.startswith("k_arr"):
            acc[n][r["Counter_Name"]]+=float(r["Counter_Value"])
    os.remove(f)
for n in acc:
    print(n, " ".join("%s=%.3g"%(k.replace("SQ_",""),v) for k,v in sorted(acc[n].items())))
PY
