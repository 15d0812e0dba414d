# rocprofv3 kernel statistics of one bench configuration: tools/prof_one.sh <name> <bench arguments...>
# Output: $OUT (default out/<round>)/<name>_{bench.json,kernel_stats.csv}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT; R=${R:-r05}
OUT=${OUT:-out/$R}; mkdir -p $OUT
name=$1; shift
python3 bench.py --full --no-cpu-baseline --no-ratio320 --no-other-entry --steps 4 --warmup 2 "$@" > $OUT/${name}_bench.json 2> $OUT/${name}_bench.err || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$name -- python3 bench.py --full --no-cpu-baseline --no-ratio320 --no-other-entry --steps 4 --warmup 2 "$@" > $OUT/${name}_prof.log 2>&1 || exit 1
f=$(ls $OUT/prof_$name/*/*kernel_stats.csv | head -1); cp $f $OUT/${name}_kernel_stats.csv; rm -rf $OUT/prof_$name
python3 -c "
import json; d=json.loads(open('$OUT/${name}_bench.json').read().strip().splitlines()[-1]); r=d['roofline']
print('$name', d['value'], d['ms_per_step'], d['updates_per_sec'], r['kernel'][:40], r['achieved'], r['frac'], r['avg_us'])"
