# Top-level build: libnbx.so (HIP kernels + C-ABI, gfx950 only), the drop-in nbody.x, the oracle.
HIPCC ?= hipcc
ARCH  ?= gfx950
PKG    = nbody-demo-2023_amd
CSRC   = $(PKG)/csrc
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -fhip-fp32-correctly-rounded-divide-sqrt

all: lib host oracle

lib: $(PKG)/libnbx.so

$(PKG)/nbx_api.o: $(CSRC)/nbx_api.hip $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_kernels.hpp $(CSRC)/nbx_jlane.hpp $(CSRC)/nbx_pair.hpp $(CSRC)/nbx_sgpr_loop.inc $(CSRC)/nbx_jlane_loop.inc include/nbx.h include/nbx_diag.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_group.o: $(CSRC)/nbx_group.hip $(CSRC)/nbx_shares.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_watchdog.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_kick.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_diag.o: $(CSRC)/nbx_diag.hip $(CSRC)/nbx_diag_kernels.hpp $(CSRC)/nbx_diag_body.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_ensemble.o: $(CSRC)/nbx_ensemble.hip $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_ensemble_kernels.hpp $(CSRC)/nbx_jlane.hpp $(CSRC)/nbx_jlane_loop.inc $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_ensemble_diag.o: $(CSRC)/nbx_ensemble_diag.hip $(CSRC)/nbx_ensemble_diag_kernels.hpp $(CSRC)/nbx_diag_body.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ensemble_diag.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_ragged.o: $(CSRC)/nbx_ragged.hip $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_ragged_kernels.hpp $(CSRC)/nbx_jlane.hpp $(CSRC)/nbx_jlane_loop.inc $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ragged.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_ragged_diag.o: $(CSRC)/nbx_ragged_diag.hip $(CSRC)/nbx_ragged_diag_kernels.hpp $(CSRC)/nbx_diag_body.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ragged.h include/nbx_ragged_diag.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_batch_accel.o: $(CSRC)/nbx_batch_accel.hip $(CSRC)/nbx_batch_accel_kernels.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_jlane.hpp $(CSRC)/nbx_jlane_loop.inc $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_batch_accel.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_kick.o: $(CSRC)/nbx_kick.hip $(CSRC)/nbx_kick_kernels.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_jlane.hpp $(CSRC)/nbx_jlane_loop.inc $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_kick.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_timescale.o: $(CSRC)/nbx_timescale.hip $(CSRC)/nbx_timescale_kernels.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_timescale.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_field.o: $(CSRC)/nbx_field.hip $(CSRC)/nbx_field_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_field.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_neighbours.o: $(CSRC)/nbx_neighbours.hip $(CSRC)/nbx_neighbours_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_neighbours.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_paircount.o: $(CSRC)/nbx_paircount.hip $(CSRC)/nbx_paircount_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_paircount.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_tracers.o: $(CSRC)/nbx_tracers.hip $(CSRC)/nbx_tracers_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_tracers.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_knn.o: $(CSRC)/nbx_knn.hip $(CSRC)/nbx_knn_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_knn.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_fof.o: $(CSRC)/nbx_fof.hip $(CSRC)/nbx_fof_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_fof.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_binaries.o: $(CSRC)/nbx_binaries.hip $(CSRC)/nbx_binaries_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_binaries.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_tidal.o: $(CSRC)/nbx_tidal.hip $(CSRC)/nbx_tidal_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_tidal.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_clumps.o: $(CSRC)/nbx_clumps.hip $(CSRC)/nbx_clumps_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_clumps.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_nlist.o: $(CSRC)/nbx_nlist.hip $(CSRC)/nbx_nlist_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_nlist_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_nlist.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_jerk.o: $(CSRC)/nbx_jerk.hip $(CSRC)/nbx_jerk_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_jerk.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_hermite.o: $(CSRC)/nbx_hermite.hip $(CSRC)/nbx_hermite_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_hermite.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_advance.o: $(CSRC)/nbx_advance.hip $(CSRC)/nbx_advance_kernels.hpp $(CSRC)/nbx_analysis.hpp $(CSRC)/nbx_tilewalk.hpp $(CSRC)/nbx_field_shape.hpp $(CSRC)/nbx_ensemble_internal.hpp $(CSRC)/nbx_ragged_internal.hpp $(CSRC)/nbx_batch.hpp $(CSRC)/nbx_internal.hpp $(CSRC)/nbx_object.hpp $(CSRC)/nbx_plan.hpp $(CSRC)/nbx_diag_shape.hpp $(CSRC)/nbx_pair.hpp include/nbx.h include/nbx_diag.h include/nbx_ensemble.h include/nbx_ragged.h include/nbx_advance.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(PKG)/nbx_ic.o: $(CSRC)/nbx_ic.cpp include/nbx.h
	$(HIPCC) -O2 -std=c++17 -fPIC -Wall -ffp-contract=off -c $< -o $@
$(PKG)/libnbx.so: $(PKG)/nbx_api.o $(PKG)/nbx_group.o $(PKG)/nbx_diag.o $(PKG)/nbx_ensemble.o $(PKG)/nbx_ensemble_diag.o $(PKG)/nbx_ragged.o $(PKG)/nbx_ragged_diag.o $(PKG)/nbx_batch_accel.o $(PKG)/nbx_kick.o $(PKG)/nbx_timescale.o $(PKG)/nbx_field.o $(PKG)/nbx_neighbours.o $(PKG)/nbx_paircount.o $(PKG)/nbx_tracers.o $(PKG)/nbx_knn.o $(PKG)/nbx_fof.o $(PKG)/nbx_binaries.o $(PKG)/nbx_tidal.o $(PKG)/nbx_clumps.o $(PKG)/nbx_nlist.o $(PKG)/nbx_jerk.o $(PKG)/nbx_hermite.o $(PKG)/nbx_advance.o $(PKG)/nbx_ic.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl

host: lib
	$(MAKE) -C $(PKG)/host

oracle:
	$(MAKE) -C oracle

run: host
	$(PKG)/host/nbody.x

clean:
	rm -f $(PKG)/*.o $(PKG)/libnbx.so
	$(MAKE) -C $(PKG)/host clean
	$(MAKE) -C oracle clean

.PHONY: all lib host oracle run clean
