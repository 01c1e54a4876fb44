# Kernel traces of bench.py over several library builds (per-kernel average durations):
# LIBS="lidar_slam_amd/variants/lib_a.so lidar_slam_amd/liblidarslam.so" bash tools/kt_libs.sh
cd "$(dirname "$0")/.."; OUT=${LSLAM_OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
i=0
for lib in $LIBS; do
  i=$((i+1))
  export LSLAM_ALLOW_STALE=1 LSLAM_LIB=$PWD/$lib
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $OUT/kt_$i -o kt --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-alone --steps 20 --warmup 3 > $OUT/kt_$i.log 2>&1 || { tail -5 $OUT/kt_$i.log; exit 1; }
  echo "== $lib"
  cut -d, -f1-4 $OUT/kt_$i/kt_kernel_stats.csv | head -12
done
