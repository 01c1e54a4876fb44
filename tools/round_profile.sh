# Everything profiles/<tag>_* holds, in one GPU call; each step time-limited, stop at the first failure.
# Usage: tools/round_profile.sh <tag>   (then: python tools/profile_summary.py <tag>)
cd "$(dirname "$0")/.."; OUT=${LSLAM_OUT:-bench_out}; mkdir -p $OUT
TAG=${1:?tag}
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -1 $OUT/gpu_tests.log
timeout -k 10 400 python -u bench.py --full > $OUT/bench.log 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
tail -1 $OUT/bench.log
bash tools/profile_session.sh $TAG || exit 1
timeout -k 10 300 python -u tools/c5bench.py --scans 4096 --reps 2 > $OUT/c5.json 2> $OUT/c5.err || { tail -20 $OUT/c5.err; exit 1; }
cat $OUT/c5.json
timeout -k 10 300 python -u tools/mapbench.py > $OUT/mapbench.json 2> $OUT/mapbench.err || { tail -20 $OUT/mapbench.err; exit 1; }
cat $OUT/mapbench.json
# producer window segments (diagnostic variant lib_wstamps.so) and consensus phases (liblidarslam_stamps.so;
# Philox hypotheses: in mt19937 mode the producer's own stamps share the debug buffer)
if [ -f lidar_slam_amd/variants/lib_wstamps.so ]; then
  LSLAM_LIB=$PWD/lidar_slam_amd/variants/lib_wstamps.so timeout -k 10 120 python -u tools/wstamps.py > $OUT/${TAG}_wstamps.json 2> $OUT/ws.err || { tail -5 $OUT/ws.err; exit 1; }
  cat $OUT/${TAG}_wstamps.json
fi
if [ -f lidar_slam_amd/liblidarslam_stamps.so ]; then
  timeout -k 10 120 python -u tools/chunkstamps.py 4096 philox > $OUT/${TAG}_chunkstamps.json 2> $OUT/cs.err || { tail -5 $OUT/cs.err; exit 1; }
  cat $OUT/${TAG}_chunkstamps.json
fi
