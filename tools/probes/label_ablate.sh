# The label kernel's duration under rocprofv3 for variant builds of the library:  tools/probes/label_ablate.sh <variant> ...
#   product                                   k_label_reads_lds, the kernel the product launches
#   product-lds0                              the product library under FSEG_LABEL_LDS=0: k_label_reads as it was
#   nosearch / noloop / nostore / noexon      tools/build_variant.sh <name> -DFSEG_LAB_NOSEARCH / _NOLOOP / _NOSTORE / _NOEXON: diagnostic
#                                             builds of k_label_reads (wrong results, timing only), run under FSEG_LABEL_LDS=0
#   anything else                             freddie_amd/libfreddie_seg_<variant>.so as it is (WORKLOAD=config5, FREDDIE_BENCH_BATCH_READS=250000 ...)
# median / min / max over a run's launches in profiles/label_lds.txt were taken from the kernel trace of the same runs.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${OUT:-$TMPDIR/label_ablate}; mkdir -p $O      # where the traces and logs go
for v in "$@"; do
  L=$PWD/freddie_amd/libfreddie_seg_$v.so; LDS=
  case $v in product) L=$PWD/freddie_amd/libfreddie_seg.so;; product-lds0) L=$PWD/freddie_amd/libfreddie_seg.so; LDS=0;; nosearch|noloop|nostore|noexon) LDS=0;; esac
  FSEG_LABEL_LDS=$LDS FSEG_LIB=$L FSEG_NO_FORK=1 timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/sm_$v -o p -- python3 tools/replay_probe.py --workload ${WORKLOAD:-config4} > $O/sm_$v.log 2>&1 || exit 1
  python3 - <<P
import csv
for r in csv.DictReader(open('$O/sm_$v/p_kernel_stats.csv')):
    if 'k_label_reads' in r['Name']: print('$v', r['Name'].split('(')[0], r['Calls'], round(float(r['AverageNs'])/1e3, 1), 'us')
P
done
