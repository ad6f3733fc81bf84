#!/bin/bash
# build_variant.sh NAME [ENV=VALUE ...] -- an A/B build of libnbx.so with other generator settings (tools/gen_sgpr_loop.py reads its
# knobs from the environment): copies csrc/, regenerates the loop include there, links tools/ab/NAME/libnbx.so.  Run with
# NBX_LIB=tools/ab/NAME/libnbx.so.  Development harness, not part of the product.
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$here/..
name=$1; shift
dir=$here/ab/$name
rm -rf "$dir"; mkdir -p "$dir/pkg/csrc" "$dir/include"
cp "$root"/nbody-demo-2023_amd/csrc/* "$dir/pkg/csrc/"
cp "$root"/include/nbx.h "$root"/include/nbx_diag.h "$root"/include/nbx_ensemble.h "$root"/include/nbx_ensemble_diag.h \
   "$root"/include/nbx_ragged.h "$root"/include/nbx_ragged_diag.h "$root"/include/nbx_batch_accel.h "$root"/include/nbx_kick.h \
   "$root"/include/nbx_timescale.h "$root"/include/nbx_field.h "$root"/include/nbx_neighbours.h \
   "$root"/include/nbx_paircount.h "$root"/include/nbx_tracers.h "$root"/include/nbx_knn.h "$root"/include/nbx_fof.h \
   "$root"/include/nbx_binaries.h "$root"/include/nbx_tidal.h "$root"/include/nbx_clumps.h "$root"/include/nbx_nlist.h \
   "$root"/include/nbx_jerk.h "$root"/include/nbx_hermite.h "$root"/include/nbx_advance.h "$dir/include/"
env "$@" python3 "$here/gen_sgpr_loop.py" "$dir/pkg/csrc/nbx_sgpr_loop.inc"
flags="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -fhip-fp32-correctly-rounded-divide-sqrt"
# csrc includes "../../include/nbx_diag.h" (which includes nbx.h) relative to pkg/csrc -> $dir/include
(cd "$dir/pkg/csrc" && hipcc $flags -c nbx_api.hip -o ../nbx_api.o && hipcc $flags -c nbx_group.hip -o ../nbx_group.o &&
 hipcc $flags -c nbx_diag.hip -o ../nbx_diag.o && hipcc $flags -c nbx_ensemble.hip -o ../nbx_ensemble.o &&
 hipcc $flags -c nbx_ensemble_diag.hip -o ../nbx_ensemble_diag.o &&
 hipcc $flags -c nbx_ragged.hip -o ../nbx_ragged.o && hipcc $flags -c nbx_ragged_diag.hip -o ../nbx_ragged_diag.o &&
 hipcc $flags -c nbx_batch_accel.hip -o ../nbx_batch_accel.o && hipcc $flags -c nbx_kick.hip -o ../nbx_kick.o &&
 hipcc $flags -c nbx_timescale.hip -o ../nbx_timescale.o &&
 hipcc $flags -c nbx_field.hip -o ../nbx_field.o &&
 hipcc $flags -c nbx_neighbours.hip -o ../nbx_neighbours.o &&
 hipcc $flags -c nbx_paircount.hip -o ../nbx_paircount.o &&
 hipcc $flags -c nbx_tracers.hip -o ../nbx_tracers.o &&
 hipcc $flags -c nbx_knn.hip -o ../nbx_knn.o &&
 hipcc $flags -c nbx_fof.hip -o ../nbx_fof.o &&
 hipcc $flags -c nbx_binaries.hip -o ../nbx_binaries.o &&
 hipcc $flags -c nbx_tidal.hip -o ../nbx_tidal.o &&
 hipcc $flags -c nbx_clumps.hip -o ../nbx_clumps.o &&
 hipcc $flags -c nbx_nlist.hip -o ../nbx_nlist.o &&
 hipcc $flags -c nbx_jerk.hip -o ../nbx_jerk.o &&
 hipcc $flags -c nbx_hermite.hip -o ../nbx_hermite.o &&
 hipcc $flags -c nbx_advance.hip -o ../nbx_advance.o &&
 hipcc -O2 -std=c++17 -fPIC -ffp-contract=off -c nbx_ic.cpp -o ../nbx_ic.o)
hipcc --offload-arch=gfx950 -shared -fPIC -o "$dir/libnbx.so" "$dir"/pkg/*.o -ldl
echo "built $dir/libnbx.so"
