#!/bin/bash
# Build libwfae.so for gfx950 in-tree (cross-compiles without a GPU).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -Wno-unused-result"
mkdir -p build
pids=()
for f in api gemm dconv norm_act loss ssim skill transformer wino forecast dlinear prediff convae aekl aekl_bwd lpips vit c1conv splitgemm c1b c1w g3b c1r c1rb c1n c1wd c1ws augment vil_pool c3s2 convattn resae resae_bwd panels latent_cache linear_rowinv verify; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ common.h -nt build/$f.o ] || [ resae_common.h -nt build/$f.o ] || [ ../../include/wfae.h -nt build/$f.o ] || [ ../../include/wfae_verify.h -nt build/$f.o ]; then
    $HIPCC $FLAGS -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libwfae.so build/api.o build/gemm.o build/dconv.o build/norm_act.o build/loss.o build/ssim.o build/skill.o build/transformer.o build/wino.o build/forecast.o build/dlinear.o build/prediff.o build/convae.o build/aekl.o build/aekl_bwd.o build/lpips.o build/vit.o build/c1conv.o build/splitgemm.o build/c1b.o build/c1w.o build/g3b.o build/c1r.o build/c1rb.o build/c1n.o build/c1wd.o build/c1ws.o build/augment.o build/vil_pool.o build/c3s2.o build/convattn.o build/resae.o build/resae_bwd.o build/panels.o build/latent_cache.o build/linear_rowinv.o build/verify.o
echo "built $(cd .. && pwd)/libwfae.so"
