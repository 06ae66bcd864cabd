#!/bin/bash
# blur tile shape x staging form (a -DPWN_BLUR_SWEEP build, PWN_DBG_BLUR_TW / _TH / _BATCH), judged by the frame rate on two streams
cd "$GRAFT_REPO_ROOT"
O=gpurun_out/r3_w; mkdir -p $O
export PWNHIP_LIB=$PWD/pwnfps_amd/libpwnhip_sweep.so
for rep in 1 2; do
for cfg in "128 32 0" "128 32 1" "128 16 1" "128 8 1" "64 32 0" "64 32 1" "64 16 0" "64 16 1" "64 8 1" "32 32 1"; do set -- $cfg
  export PWN_DBG_BLUR_TW=$1 PWN_DBG_BLUR_TH=$2 PWN_DBG_BLUR_BATCH=$3
  line="tile $1x$2 batch $3:"
  for wh in "3840 2160 pwnfps_level" "1280 720 pwnfps_level" "1920 1080 synth64" "7680 4320 synth256"; do set -- $wh
    r=$(python bench.py --full --no-cpu-baseline --min-time 1 --no-d2h --width $1 --height $2 --level $3 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('%.0f (blur %.4f)' % (d['value'], d['blur_roofline']['avg_launch_ms']))")
    line="$line  $1x$2 $r"
  done
  s=$(python3 tools/strip_time.py 8 2>&1 | grep -v amdgpu | tail -1 | sed 's/.*sum over strips of the 2-stream figure //')
  echo "$line  strips8 $s"
done; done > $O/blur_sweep.txt 2>&1
cat $O/blur_sweep.txt
