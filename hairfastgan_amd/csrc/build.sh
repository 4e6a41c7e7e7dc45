#!/bin/bash
# Builds libhairfast_hip.so in-tree for gfx950 (MI355X).  hipcc cross-compiles
# without a GPU.  Usage: hairfastgan_amd/csrc/build.sh [extra hipcc flags]
# Out-of-date objects are compiled concurrently (convh.hip alone takes ~1 min).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC $*"
OBJS=""
PIDS=""
for f in api elementwise upfirdn2d style torgb modconv convh convh_enc encoder_ops sean vit gemm_h stem convrow; do
  DEPS="$f.hip hf_common.h conv_common.h ../../include/hairfast_hip.h"
  [ $f = encoder_ops ] && DEPS="$DEPS poisson.h align.h paste.h export.h codec_common.h png.h jpeg.h jpeg_decode.h png_decode.h metric_common.h frechet.h lpips.h ssim.h identity.h inception.h"  # what it includes
  [ $f = gemm_h ] && DEPS="$DEPS conv_rect.h"
  STALE=""
  for d in $DEPS; do
    [ $d -nt $f.o ] && STALE=1
  done
  if [ ! -f $f.o ] || [ -n "$STALE" ]; then
    $HIPCC $FLAGS -c $f.hip -o $f.o &
    PIDS="$PIDS $!"
  fi
  OBJS="$OBJS $f.o"
done
for p in $PIDS; do
  wait $p  # set -e: a failed compile aborts the build
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libhairfast_hip.so $OBJS
echo built $(pwd)/libhairfast_hip.so
