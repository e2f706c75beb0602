#!/bin/bash
# Build libmvae_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
# `build.sh tune` builds the diagnostic variant libmvae_hip_tune.so (-DMVAE_TUNING: MVAE_DBG can skip the main loop / the epilogue of
# the step kernels -- wrong results, timing decompositions only).  The product library has no such hook.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
# latent.hip's pairwise kernel keeps a z row in registers, latent_knn.hip's scan a table row: SLP-packed f32 pairs would add operand moves
# and registers, not speed
xflags() { { [ "$1" = latent ] || [ "$1" = latent_knn ]; } && echo "-fno-slp-vectorize" || true; }
mkdir -p build
if [ "${1:-}" = "tune" ]; then
  mkdir -p build/tune ../../tests/tuning/lib
  pids=()
  for f in gemm rnn rnn_rowres rnn_persist rnn_persist_bwd selfies smiles_aromatize fragment_smiles fragment scaffold_smiles smiles_substruct smiles_canon smiles_rewrite kekule moses_decode scaffold fingerprint smiles_graph elementwise edit_distance latent_knn corpus_index conv latent capi; do
    $HIPCC $FLAGS $(xflags $f) -DMVAE_TUNING -c $f.hip -o build/tune/$f.o &
    pids+=($!)
  done
  for p in "${pids[@]}"; do wait $p; done
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o ../../tests/tuning/lib/libmvae_hip_tune.so build/tune/gemm.o build/tune/rnn.o build/tune/rnn_rowres.o build/tune/rnn_persist.o build/tune/rnn_persist_bwd.o build/tune/selfies.o build/tune/smiles_aromatize.o build/tune/fragment_smiles.o build/tune/fragment.o build/tune/scaffold_smiles.o build/tune/smiles_substruct.o build/tune/smiles_canon.o build/tune/smiles_rewrite.o build/tune/kekule.o build/tune/moses_decode.o build/tune/scaffold.o build/tune/fingerprint.o build/tune/smiles_graph.o build/tune/elementwise.o build/tune/edit_distance.o build/tune/latent_knn.o build/tune/corpus_index.o build/tune/conv.o build/tune/latent.o build/tune/capi.o
  echo "built $(cd ../../tests/tuning/lib && pwd)/libmvae_hip_tune.so"
  exit 0
fi
pids=()
for f in gemm rnn rnn_rowres rnn_persist rnn_persist_bwd selfies smiles_aromatize fragment_smiles fragment scaffold_smiles smiles_substruct smiles_canon smiles_rewrite kekule moses_decode scaffold fingerprint smiles_graph elementwise edit_distance latent_knn corpus_index conv latent capi; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ common.hpp -nt build/$f.o ] || [ tile.hpp -nt build/$f.o ] || [ tile_pipe.hpp -nt build/$f.o ] || [ kernels.hpp -nt build/$f.o ] || [ persist_common.hpp -nt build/$f.o ] || [ smiles_syntax.hpp -nt build/$f.o ] || [ smiles_graph.hpp -nt build/$f.o ] || [ smiles_rounds.hpp -nt build/$f.o ] || [ smiles_writer.hpp -nt build/$f.o ] || [ smiles_canon.hpp -nt build/$f.o ] || [ scaffold_sets.hpp -nt build/$f.o ] || [ graph_key.hpp -nt build/$f.o ] || [ fragment_sets.hpp -nt build/$f.o ] || [ smiles_cut.hpp -nt build/$f.o ] || [ kekule.hpp -nt build/$f.o ] || [ selfies.hpp -nt build/$f.o ] || [ ../../include/mvae.h -nt build/$f.o ] || [ -n "$(find . -maxdepth 1 -name '*.hpp' -newer build/$f.o)" ]; then
    # (the last test covers every header of this directory, the named ones and any added later)
    # -Rpass-analysis: per-kernel VGPR / scratch / spill figures go to build/$f.usage.txt (tests assert that no kernel uses scratch)
    $HIPCC $FLAGS $(xflags $f) -Rpass-analysis=kernel-resource-usage -c $f.hip -o build/$f.o 2> build/$f.usage.txt &
    pids+=($!)
  fi
done
rc=0
for p in "${pids[@]:-}"; do [ -n "$p" ] && { wait $p || rc=1; }; done
if [ $rc -ne 0 ]; then grep -h -B2 -A6 "error" build/*.usage.txt | head -60; exit 1; fi
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libmvae_hip.so build/gemm.o build/rnn.o build/rnn_rowres.o build/rnn_persist.o build/rnn_persist_bwd.o build/selfies.o build/smiles_aromatize.o build/fragment_smiles.o build/fragment.o build/scaffold_smiles.o build/smiles_substruct.o build/smiles_canon.o build/smiles_rewrite.o build/kekule.o build/moses_decode.o build/scaffold.o build/fingerprint.o build/smiles_graph.o build/elementwise.o build/edit_distance.o build/latent_knn.o build/corpus_index.o build/conv.o build/latent.o build/capi.o
echo "built $(cd .. && pwd)/libmvae_hip.so"
