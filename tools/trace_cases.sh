#!/bin/bash
# The case list of DESIGN §4.15 / §4.17 through tools/launch_trace.py, one process per configuration (the package reads
# its HAIRFAST_* switches at import).  Needs no GPU; needs tests/hipsim/libhairfast_sim.so of ROOT (tests/hipsim/build_sim.sh).
#   tools/trace_cases.sh dry|plan ROOT OUTDIR
# dry:  OUTDIR/NN.calls = the C calls.   plan: also OUTDIR/NN.plan = every kernel launch's plan, and the sweep.
# Run it on a `git worktree` of the base revision (plan: with this revision's tests/hipsim and tools/launch_trace.py
# copied over it) and on the working tree, then `diff -r` the two directories.
set -e
MODE=$1; ROOT=$(cd "$2" && pwd); OUT=$3
[ "$MODE" = dry ] || [ "$MODE" = plan ] || { echo "usage: $0 dry|plan ROOT OUTDIR" >&2; exit 2; }
mkdir -p "$OUT"
GEN="gen:8 gen:3 gen:1 gen:3:0:3 gen:1:0:3 gen:3:3:3 gen:1:3:3 gen:1:4:8 gen:1:5:8"
n=0
run() {  # run "ENV=VALUE ..." [--hook] CASE...   ("": the defaults)
  local envs=$1; shift
  n=$((n + 1))
  local id; id=$(printf %02d $n)
  echo "$id: $envs $*"
  if [ "$MODE" = plan ]; then
    env $envs python "$ROOT/tools/launch_trace.py" --root "$ROOT" --plan "$OUT/$id.plan" --out "$OUT/$id.calls" "$@"
  else
    env $envs python "$ROOT/tools/launch_trace.py" --root "$ROOT" --dry --out "$OUT/$id.calls" "$@"
  fi
}
run "" $GEN embed
run "HAIRFAST_CONV_PRECISION=f16" gen:16 embed
run "HAIRFAST_CONV_PRECISION=f32" gen:2
run "HAIRFAST_DETERMINISTIC=0" gen:8 gen:1
run "" --hook gen:8
run "HAIRFAST_IMAGE_FUSE=0" gen:8
run "HAIRFAST_SMALL_UP_FUSED=0" gen:8
run "HAIRFAST_FUSE_BLUR_MIN_H=16" gen:8
run "HAIRFAST_ENC_PRESPLIT=none" embed
run "HAIRFAST_ENC_PRESPLIT=heads" embed
run "HAIRFAST_GEMM_H=0" embed
run "HAIRFAST_CONV_PAIR=0" embed
run "HAIRFAST_UNIT_CHAIN=0" embed
wc -l "$OUT"/* | tail -1
