#!/bin/bash
# Proves that a source-only refactor of the HIP library leaves its machine code unchanged.  Compiles every source of
# hairfastgan_amd/csrc/build.sh at BASE_REV (a temporary git worktree) and in the working tree, device and host side
# apart, and compares per source:
#   - the gfx950 disassembly (llvm-objdump -d, addresses and comments stripped: the raw code-object bytes differ
#     between two compiles of the same source),
#   - the code-object notes (llvm-readelf --notes: registers, LDS, scratch, kernarg size),
#   - the disassembly of the host object's .text.
# Usage: tools/compare_isa.sh BASE_REV [extra hipcc flags]   Exit status 0: all identical.  Needs no GPU.
set -e
[ -n "$1" ] || { echo "usage: $0 BASE_REV [hipcc flags]" >&2; exit 2; }
BASE=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
LLVM=${LLVM:-/opt/rocm/llvm/bin}
SRCS="api elementwise upfirdn2d style torgb modconv convh convh_enc encoder_ops sean vit gemm_h stem convrow"
W=$(mktemp -d -t compare_isa.XXXXXX)
trap 'git -C "$ROOT" worktree remove --force "$W/base_tree" >/dev/null 2>&1; rm -rf "$W"' EXIT
git -C "$ROOT" worktree add --detach "$W/base_tree" "$BASE" >/dev/null

# dump <csrc dir> <out dir> [flags]: device disassembly + notes and host .text disassembly of every source
dump() {
  local src=$1 out=$2; shift 2
  mkdir -p "$out"
  for f in $SRCS; do
    (
      cd "$src"
      $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" --offload-device-only -c $f.hip -o "$out/$f.dev.o"
      $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" --offload-host-only -c $f.hip -o "$out/$f.host.o"
      cd "$out"
      $LLVM/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
        --input=$f.dev.o --output=$f.gfx950.co
      $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $f.gfx950.co | sed -e 's#[[:space:]]*//.*$##' \
        > $f.dev.s
      $LLVM/llvm-readelf --notes $f.gfx950.co > $f.notes
      $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr -j .text $f.host.o | sed -e 's#[[:space:]]*//.*$##' \
        > $f.host.s
      rm -f $f.dev.o $f.host.o $f.gfx950.co
    ) &
  done
  wait
}

dump "$W/base_tree/hairfastgan_amd/csrc" "$W/base" "$@"
dump "$ROOT/hairfastgan_amd/csrc" "$W/new" "$@"
status=0
for f in $SRCS; do
  for k in dev.s notes host.s; do
    [ -s "$W/base/$f.$k" ] && [ -s "$W/new/$f.$k" ] || { echo "$f.$k: missing (compile failed?)"; status=1; continue; }
    if cmp -s "$W/base/$f.$k" "$W/new/$f.$k"; then
      echo "$f.$k: identical ($(wc -l < "$W/new/$f.$k") lines)"
    else
      echo "$f.$k: DIFFERS"; diff "$W/base/$f.$k" "$W/new/$f.$k" | head -20; status=1
    fi
  done
done
exit $status
