"""ctypes binding of libnbx.so (include/nbx.h) -- used by tests/, bench.py and __graft_entry__.

Thin by design: every method is one C-ABI call.  There is NO fallback: if libnbx.so is missing
the import of the library fails loudly, and without a HIP device nbx_create() returns
NBX_ERR_DEVICE which is raised as NbxError.
"""
import ctypes
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NBX_LIB") or os.path.join(_HERE, "libnbx.so")

NBX_OK, NBX_ERR_ARG, NBX_ERR_DEVICE, NBX_ERR_STATE, NBX_ERR_ALLOC = 0, -1, -2, -3, -4
ORDER_AUTO, ORDER_REFERENCE, ORDER_TREE = 0, 1, 2
LOOP_AUTO, LOOP_CXX, LOOP_ASM, LOOP_ASM_TS, LOOP_ASM_PF = 0, 1, 2, 3, 4
KERNEL_AUTO, KERNEL_LDS, KERNEL_SGPR, KERNEL_SGPRW, KERNEL_EXACT, KERNEL_EXACT_FMA, KERNEL_JLANE = 0, 1, 2, 3, 4, 5, 6

# every symbol include/nbx.h declares (tests check the library exports each of them)
SYMBOLS = (
    "nbx_last_error", "nbx_abi_version", "nbx_create", "nbx_destroy", "nbx_upload", "nbx_step",
    "nbx_step_trace", "nbx_step_local", "nbx_exchange_buffer", "nbx_commit", "nbx_kenergy_partial",
    "nbx_accel", "nbx_sync", "nbx_download", "nbx_ic_pos", "nbx_ic_vel", "nbx_ic_mass", "nbx_profile",
    "nbx_stats", "nbx_group_create", "nbx_group_destroy", "nbx_group_upload", "nbx_group_step", "nbx_group_download",
    "nbx_group_info", "nbx_partition", "nbx_comm_unique_id", "nbx_group_create_rank", "nbx_collective_timeout",
    "nbx_partition_weighted", "nbx_group_create_weighted", "nbx_group_shares", "nbx_tune_weights", "nbx_group_retune",
)

# the symbols of include/nbx_diag.h (physics diagnostics), kept apart from the set nbx.h declares
DIAG_SYMBOLS = ("nbx_diagnostics", "nbx_group_diagnostics")

# the symbols of include/nbx_ensemble.h (many small systems per launch), kept apart likewise
ENSEMBLE_SYMBOLS = (
    "nbx_ensemble_create", "nbx_ensemble_destroy", "nbx_ensemble_upload", "nbx_ensemble_step", "nbx_ensemble_step_trace",
    "nbx_ensemble_download", "nbx_ensemble_sync", "nbx_ensemble_profile", "nbx_ensemble_stats",
)

# the symbol of include/nbx_ensemble_diag.h (the diagnostics of every member of an ensemble in one launch), kept apart likewise
ENSEMBLE_DIAG_SYMBOLS = ("nbx_ensemble_diagnostics",)

# the symbols of include/nbx_ragged.h (systems of different size in one launch), kept apart likewise
RAGGED_SYMBOLS = (
    "nbx_ragged_create", "nbx_ragged_destroy", "nbx_ragged_upload", "nbx_ragged_step", "nbx_ragged_step_trace",
    "nbx_ragged_download", "nbx_ragged_sync", "nbx_ragged_profile", "nbx_ragged_stats",
)

# the symbol of include/nbx_ragged_diag.h (the diagnostics of every member of a ragged ensemble in one launch), kept apart likewise
RAGGED_DIAG_SYMBOLS = ("nbx_ragged_diagnostics",)

# the symbols of include/nbx_batch_accel.h (the accelerations of the members of either kind in one launch), kept apart likewise
BATCH_ACCEL_SYMBOLS = ("nbx_ensemble_accel", "nbx_ragged_accel")

# the symbols of include/nbx_kick.h (velocity-only half steps for every kind of object), kept apart likewise
KICK_SYMBOLS = ("nbx_kick", "nbx_ensemble_kick", "nbx_ragged_kick", "nbx_group_kick")

# the symbols of include/nbx_timescale.h (pair approach and free-fall rates for choosing dt), kept apart likewise
TIMESCALE_SYMBOLS = ("nbx_timescale", "nbx_ensemble_timescale", "nbx_ragged_timescale")

# the symbols of include/nbx_field.h (acceleration and potential at caller-supplied points), kept apart likewise
FIELD_SYMBOLS = ("nbx_field", "nbx_ensemble_field", "nbx_ragged_field")
FIELD_KEYS = ("acc_x", "acc_y", "acc_z", "phi")

# the symbols of include/nbx_neighbours.h (nearest neighbour and radius count of every body), kept apart likewise
NEIGHBOUR_SYMBOLS = ("nbx_neighbours", "nbx_ensemble_neighbours", "nbx_ragged_neighbours")
NEIGHBOUR_KEYS = ("index", "r2", "within")

# the symbols of include/nbx_paircount.h (pairs within each of a list of radii), kept apart likewise
PAIRCOUNT_SYMBOLS = ("nbx_paircount", "nbx_ensemble_paircount", "nbx_ragged_paircount")
PAIRCOUNT_MAX_RADII = 256

# the symbols of include/nbx_tracers.h (resident test particles that step with the bodies), kept apart likewise
TRACER_SYMBOLS = (
    "nbx_tracers_upload", "nbx_tracers_download", "nbx_tracers_count", "nbx_tracers_step", "nbx_tracers_kick",
    "nbx_ensemble_tracers_upload", "nbx_ensemble_tracers_download", "nbx_ensemble_tracers_count", "nbx_ensemble_tracers_step",
    "nbx_ensemble_tracers_kick",
    "nbx_ragged_tracers_upload", "nbx_ragged_tracers_download", "nbx_ragged_tracers_count", "nbx_ragged_tracers_step",
    "nbx_ragged_tracers_kick",
)
TRACER_MAX = 1 << 22  # tracers per object: members * m

# the symbols of include/nbx_knn.h (the k nearest neighbours of every body), kept apart likewise
KNN_SYMBOLS = ("nbx_knn", "nbx_ensemble_knn", "nbx_ragged_knn")
KNN_KEYS = ("index", "r2")
KNN_MAX = 16

# the symbols of include/nbx_fof.h (friends-of-friends groups of the resident bodies), kept apart likewise
FOF_SYMBOLS = ("nbx_fof", "nbx_ensemble_fof", "nbx_ragged_fof")
FOF_KEYS = ("label", "size", "groups", "largest", "passes")
NBX_ERR_INTERNAL = -5  # include/nbx_fof.h: an invariant of the library did not hold
EPS2 = float(np.float32(1e-3))  # the library's softening, squared: (float)1.e-3f, widened (what every r2 carries)

# the symbols of include/nbx_binaries.h (most bound partner and bound count of every body), kept apart likewise
BINARIES_SYMBOLS = ("nbx_binaries", "nbx_ensemble_binaries", "nbx_ragged_binaries")
BINARIES_KEYS = ("partner", "energy", "bound")
# the symbols of include/nbx_tidal.h (the tidal tensor at caller-supplied points and at the bodies), kept apart likewise
TIDAL_SYMBOLS = ("nbx_tidal", "nbx_ensemble_tidal", "nbx_ragged_tidal",
                 "nbx_tidal_bodies", "nbx_ensemble_tidal_bodies", "nbx_ragged_tidal_bodies")
TIDAL_KEYS = ("t_xx", "t_xy", "t_xz", "t_yy", "t_yz", "t_zz")
# the symbols of include/nbx_clumps.h (clumps under a caller-supplied label: members, mass, centre, velocity, potential, energy)
CLUMPS_SYMBOLS = ("nbx_clumps", "nbx_ensemble_clumps", "nbx_ragged_clumps")
CLUMPS_KEYS = ("members", "gm", "centre_x", "centre_y", "centre_z", "velocity_x", "velocity_y", "velocity_z", "phi", "energy")
# the symbols of include/nbx_nlist.h (every body's neighbours within a radius, as a list), kept apart likewise
NLIST_SYMBOLS = ("nbx_nlist", "nbx_ensemble_nlist", "nbx_ragged_nlist")
NLIST_KEYS = ("offsets", "index", "r2", "total")
NLIST_MAX_CAPACITY = 1 << 28  # entries per call
NLIST_FIRST_GUESS = 16        # entries per body nlist() tries before it asks again with the exact total
GRAV = float(np.float32(6.67259e-11))  # the library's G: (float)6.67259e-11f, widened
# the symbols of include/nbx_jerk.h (the acceleration of every body and its time derivative), kept apart likewise
JERK_SYMBOLS = ("nbx_jerk", "nbx_ensemble_jerk", "nbx_ragged_jerk")
JERK_KEYS = ("acc_x", "acc_y", "acc_z", "jerk_x", "jerk_y", "jerk_z")
# the symbols of include/nbx_hermite.h (the device-resident fourth-order Hermite stepper), kept apart likewise
HERMITE_SYMBOLS = ("nbx_hermite_step", "nbx_ensemble_hermite_step", "nbx_ragged_hermite_step")
# the symbols of include/nbx_advance.h (adaptive power-of-two time steps chosen on the device), kept apart likewise
ADVANCE_SYMBOLS = ("nbx_advance", "nbx_ensemble_advance", "nbx_ragged_advance", "nbx_clock", "nbx_ensemble_clock", "nbx_ragged_clock")


class NbxError(RuntimeError):
    def __init__(self, code, where, text):
        super().__init__("%s failed (%d): %s" % (where, code, text))
        self.code = code


class Opts(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("device", ctypes.c_int32), ("stream", ctypes.c_void_p),
        ("i_begin", ctypes.c_int32), ("i_count", ctypes.c_int32), ("n_alloc", ctypes.c_int32),
        ("bodies_per_lane", ctypes.c_int32), ("j_split", ctypes.c_int32), ("kernel_variant", ctypes.c_int32),
        ("fused_epilogue", ctypes.c_int32), ("use_graph", ctypes.c_int32), ("external_stream", ctypes.c_int32),
        ("summation_order", ctypes.c_int32), ("inner_loop", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int32), ("n_alloc", ctypes.c_int32), ("i_begin", ctypes.c_int32), ("i_count", ctypes.c_int32),
        ("precision", ctypes.c_int32), ("bodies_per_lane", ctypes.c_int32), ("j_split", ctypes.c_int32),
        ("j_tile", ctypes.c_int32), ("kernel_variant", ctypes.c_int32), ("fused_epilogue", ctypes.c_int32), ("summation_order", ctypes.c_int32),
        ("force_grid_x", ctypes.c_int32), ("force_grid_y", ctypes.c_int32), ("force_block", ctypes.c_int32),
        ("cu_count", ctypes.c_int32), ("clock_mhz", ctypes.c_int32), ("steps_done", ctypes.c_int64),
        ("force_launches_timed", ctypes.c_int64), ("force_ms_total", ctypes.c_double),
        ("pairs_per_launch", ctypes.c_double), ("device_name", ctypes.c_char * 64),
        ("graph_replays", ctypes.c_int64), ("use_graph", ctypes.c_int32), ("inner_loop", ctypes.c_int32),
    ]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["device_name"] = self.device_name.decode(errors="replace")
        return d


class Diag(ctypes.Structure):
    """nbx_diag_t (include/nbx_diag.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("i_count", ctypes.c_int32), ("steps_done", ctypes.c_int64),
        ("mass", ctypes.c_double), ("kenergy", ctypes.c_double), ("potential", ctypes.c_double),
        ("momentum", ctypes.c_double * 3), ("mass_moment", ctypes.c_double * 3),
    ]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}
        d["momentum"] = list(self.momentum)
        d["mass_moment"] = list(self.mass_moment)
        d["etotal"] = self.kenergy + self.potential
        return d


class Timescale(ctypes.Structure):
    """nbx_timescale_t (include/nbx_timescale.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n", ctypes.c_int32), ("steps_done", ctypes.c_int64),
        ("approach_rate2", ctypes.c_double), ("freefall_rate2", ctypes.c_double), ("min_r2", ctypes.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class Clock(ctypes.Structure):
    """nbx_clock_t (include/nbx_advance.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n", ctypes.c_int32), ("t", ctypes.c_double), ("dt_last", ctypes.c_double),
        ("dt_next", ctypes.c_double), ("steps", ctypes.c_int64), ("floor_steps", ctypes.c_int64), ("done", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("struct_size", "reserved")}
        d["done"] = bool(d["done"])
        return d


class ClumpsOut(ctypes.Structure):
    """nbx_clumps_out_t (include/nbx_clumps.h): every pointer may be NULL."""
    _fields_ = [("members", ctypes.c_void_p), ("gm", ctypes.c_void_p), ("centre", ctypes.c_void_p * 3), ("velocity", ctypes.c_void_p * 3),
                ("phi", ctypes.c_void_p), ("energy", ctypes.c_void_p)]


class JerkOut(ctypes.Structure):
    """nbx_jerk_out_t (include/nbx_jerk.h): every pointer may be NULL."""
    _fields_ = [("acc", ctypes.c_void_p * 3), ("jerk", ctypes.c_void_p * 3)]


class EnsembleStats(ctypes.Structure):
    """nbx_ensemble_stats_t (include/nbx_ensemble.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n", ctypes.c_int32), ("n_alloc", ctypes.c_int32), ("members", ctypes.c_int32),
        ("precision", ctypes.c_int32), ("bodies_per_lane", ctypes.c_int32), ("inner_loop", ctypes.c_int32),
        ("grid_x", ctypes.c_int32), ("grid_y", ctypes.c_int32), ("block", ctypes.c_int32), ("cu_count", ctypes.c_int32),
        ("steps_done", ctypes.c_int64), ("launches_timed", ctypes.c_int64), ("step_ms_total", ctypes.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class RaggedStats(ctypes.Structure):
    """nbx_ragged_stats_t (include/nbx_ragged.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("members", ctypes.c_int32), ("precision", ctypes.c_int32), ("n_min", ctypes.c_int32),
        ("n_max", ctypes.c_int32), ("bodies_total", ctypes.c_int32), ("bodies_per_lane", ctypes.c_int32), ("inner_loop", ctypes.c_int32),
        ("grid_x", ctypes.c_int32), ("block", ctypes.c_int32), ("cu_count", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("pairs_per_step", ctypes.c_double), ("steps_done", ctypes.c_int64), ("launches_timed", ctypes.c_int64),
        ("step_ms_total", ctypes.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k not in ("struct_size", "reserved")}


_lib = None


def load():
    """Load libnbx.so (raises OSError with a build hint if it is not there)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not found: build it with `make lib` (or __graft_entry__.build()); "
                      "there is no fallback path" % LIB_PATH)
    if "torch" not in sys.modules and not os.environ.get("NBX_NO_TORCH_PRELOAD"):
        # The PyTorch-ROCm wheel bundles its own libamdhip64 / libhsa-runtime64.  Two copies of the
        # ROCm runtime cannot both initialise in one process (the second one sees no GPU), so when
        # torch is installed let it load first: libnbx.so then binds to the copy torch brought
        # (same sonames).  Stand-alone consumers (nbody.x) use /opt/rocm's copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    L.nbx_last_error.restype = ctypes.c_char_p
    L.nbx_abi_version.restype = i32
    L.nbx_create.argtypes = [ctypes.POINTER(vp), i32, i32, ctypes.POINTER(Opts)]
    L.nbx_destroy.argtypes = [vp]
    L.nbx_destroy.restype = None
    L.nbx_upload.argtypes = [vp] + [vp] * 7
    L.nbx_step.argtypes = [vp, dbl, i32, ctypes.POINTER(dbl)]
    L.nbx_step_trace.argtypes = [vp, dbl, i32, vp]
    L.nbx_step_local.argtypes = [vp, dbl]
    L.nbx_exchange_buffer.argtypes = [vp, ctypes.POINTER(vp)] + [ctypes.POINTER(ctypes.c_size_t)] * 3
    L.nbx_commit.argtypes = [vp]
    L.nbx_kenergy_partial.argtypes = [vp, ctypes.POINTER(dbl)]
    L.nbx_accel.argtypes = [vp, vp, vp, vp]
    L.nbx_sync.argtypes = [vp]
    L.nbx_download.argtypes = [vp] + [vp] * 6
    L.nbx_ic_pos.argtypes = [i32, i32, vp, vp, vp]
    L.nbx_ic_vel.argtypes = [i32, i32, vp, vp, vp]
    L.nbx_ic_mass.argtypes = [i32, i32, vp]
    L.nbx_profile.argtypes = [vp, i32]
    L.nbx_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.nbx_group_create.argtypes = [ctypes.POINTER(vp), i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(Opts)]
    L.nbx_group_destroy.argtypes = [vp]
    L.nbx_group_destroy.restype = None
    L.nbx_group_upload.argtypes = [vp] + [vp] * 7
    L.nbx_group_step.argtypes = [vp, dbl, i32, ctypes.POINTER(dbl)]
    L.nbx_group_download.argtypes = [vp] + [vp] * 6
    L.nbx_group_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, ctypes.POINTER(Stats)]
    L.nbx_partition.argtypes = [i32, i32, i32] + [ctypes.POINTER(i32)] * 5
    L.nbx_comm_unique_id.argtypes = [vp]
    L.nbx_group_create_rank.argtypes = [ctypes.POINTER(vp), i32, i32, i32, i32, vp, i32, ctypes.POINTER(Opts)]
    L.nbx_collective_timeout.argtypes = [dbl]
    pd = ctypes.POINTER(dbl)
    L.nbx_partition_weighted.argtypes = [i32, i32, pd, i32] + [ctypes.POINTER(i32)] * 4
    L.nbx_group_create_weighted.argtypes = [ctypes.POINTER(vp), i32, i32, i32, ctypes.POINTER(i32), pd, ctypes.POINTER(Opts)]
    L.nbx_group_shares.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), pd]
    L.nbx_tune_weights.argtypes = [i32, ctypes.POINTER(i32), pd, pd]
    L.nbx_group_retune.argtypes = [vp, pd, ctypes.POINTER(i32)]
    L.nbx_diagnostics.argtypes = [vp, ctypes.POINTER(Diag)]
    L.nbx_group_diagnostics.argtypes = [vp, ctypes.POINTER(Diag)]
    if hasattr(L, "nbx_ensemble_create"):  # a library built without nbx_ensemble.hip still serves everything else
        L.nbx_ensemble_create.argtypes = [ctypes.POINTER(vp), i32, i32, i32, ctypes.POINTER(Opts)]
        L.nbx_ensemble_destroy.argtypes = [vp]
        L.nbx_ensemble_destroy.restype = None
        L.nbx_ensemble_upload.argtypes = [vp, i32, i32] + [vp] * 7
        L.nbx_ensemble_step.argtypes = [vp, dbl, i32, vp]
        L.nbx_ensemble_step_trace.argtypes = [vp, dbl, i32, vp]
        L.nbx_ensemble_download.argtypes = [vp, i32, i32] + [vp] * 6
        L.nbx_ensemble_sync.argtypes = [vp]
        L.nbx_ensemble_profile.argtypes = [vp, i32]
        L.nbx_ensemble_stats.argtypes = [vp, ctypes.POINTER(EnsembleStats)]
    if hasattr(L, "nbx_ensemble_diagnostics"):  # likewise for nbx_ensemble_diag.hip
        L.nbx_ensemble_diagnostics.argtypes = [vp, i32, i32, ctypes.POINTER(Diag)]
    if hasattr(L, "nbx_ragged_create"):  # likewise for nbx_ragged.hip
        L.nbx_ragged_create.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(i32), i32, ctypes.POINTER(Opts)]
        L.nbx_ragged_destroy.argtypes = [vp]
        L.nbx_ragged_destroy.restype = None
        L.nbx_ragged_upload.argtypes = [vp, i32, i32] + [vp] * 7
        L.nbx_ragged_step.argtypes = [vp, dbl, i32, vp]
        L.nbx_ragged_step_trace.argtypes = [vp, dbl, i32, vp]
        L.nbx_ragged_download.argtypes = [vp, i32, i32] + [vp] * 6
        L.nbx_ragged_sync.argtypes = [vp]
        L.nbx_ragged_profile.argtypes = [vp, i32]
        L.nbx_ragged_stats.argtypes = [vp, ctypes.POINTER(RaggedStats)]
    if hasattr(L, "nbx_ragged_diagnostics"):  # likewise for nbx_ragged_diag.hip
        L.nbx_ragged_diagnostics.argtypes = [vp, i32, i32, ctypes.POINTER(Diag)]
    if hasattr(L, "nbx_ensemble_accel"):  # likewise for nbx_batch_accel.hip
        L.nbx_ensemble_accel.argtypes = [vp, i32, i32, vp, vp, vp]
        L.nbx_ragged_accel.argtypes = [vp, i32, i32, vp, vp, vp]
    if hasattr(L, "nbx_kick"):  # likewise for nbx_kick.hip
        L.nbx_kick.argtypes = [vp, dbl, ctypes.POINTER(dbl)]
        L.nbx_ensemble_kick.argtypes = [vp, dbl, vp]
        L.nbx_ragged_kick.argtypes = [vp, dbl, vp]
        L.nbx_group_kick.argtypes = [vp, dbl, ctypes.POINTER(dbl)]
    if hasattr(L, "nbx_timescale"):  # likewise for nbx_timescale.hip
        L.nbx_timescale.argtypes = [vp, ctypes.POINTER(Timescale)]
        L.nbx_ensemble_timescale.argtypes = [vp, i32, i32, ctypes.POINTER(Timescale)]
        L.nbx_ragged_timescale.argtypes = [vp, i32, i32, ctypes.POINTER(Timescale)]
    if hasattr(L, "nbx_field"):  # likewise for nbx_field.hip
        L.nbx_field.argtypes = [vp, i32] + [vp] * 7
        L.nbx_ensemble_field.argtypes = [vp, i32, i32, i32] + [vp] * 7
        L.nbx_ragged_field.argtypes = [vp, i32, i32, i32] + [vp] * 7
    if hasattr(L, "nbx_neighbours"):  # likewise for nbx_neighbours.hip
        L.nbx_neighbours.argtypes = [vp, dbl, vp, vp, vp]
        L.nbx_ensemble_neighbours.argtypes = [vp, i32, i32, dbl, vp, vp, vp]
        L.nbx_ragged_neighbours.argtypes = [vp, i32, i32, dbl, vp, vp, vp]
    if hasattr(L, "nbx_paircount"):  # likewise for nbx_paircount.hip
        L.nbx_paircount.argtypes = [vp, i32, vp, vp]
        L.nbx_ensemble_paircount.argtypes = [vp, i32, i32, i32, vp, vp]
        L.nbx_ragged_paircount.argtypes = [vp, i32, i32, i32, vp, vp]
    if hasattr(L, "nbx_tracers_step"):  # likewise for nbx_tracers.hip
        L.nbx_tracers_upload.argtypes = [vp, i32] + [vp] * 6
        L.nbx_tracers_download.argtypes = [vp] + [vp] * 6
        for prefix in ("nbx", "nbx_ensemble", "nbx_ragged"):
            if prefix != "nbx":
                getattr(L, prefix + "_tracers_upload").argtypes = [vp, i32, i32, i32] + [vp] * 6
                getattr(L, prefix + "_tracers_download").argtypes = [vp, i32, i32] + [vp] * 6
            getattr(L, prefix + "_tracers_count").argtypes = [vp, ctypes.POINTER(i32)]
            getattr(L, prefix + "_tracers_step").argtypes = [vp, dbl, i32, vp]
            getattr(L, prefix + "_tracers_kick").argtypes = [vp, dbl]
    if hasattr(L, "nbx_knn"):  # likewise for nbx_knn.hip
        L.nbx_knn.argtypes = [vp, i32, vp, vp]
        L.nbx_ensemble_knn.argtypes = [vp, i32, i32, i32, vp, vp]
        L.nbx_ragged_knn.argtypes = [vp, i32, i32, i32, vp, vp]
    if hasattr(L, "nbx_fof"):  # likewise for nbx_fof.hip
        L.nbx_fof.argtypes = [vp, dbl, vp, vp, vp, vp]
        L.nbx_ensemble_fof.argtypes = [vp, i32, i32, dbl, vp, vp, vp, vp]
        L.nbx_ragged_fof.argtypes = [vp, i32, i32, dbl, vp, vp, vp, vp]
    if hasattr(L, "nbx_binaries"):  # likewise for nbx_binaries.hip
        L.nbx_binaries.argtypes = [vp, vp, vp, vp]
        L.nbx_ensemble_binaries.argtypes = [vp, i32, i32, vp, vp, vp]
        L.nbx_ragged_binaries.argtypes = [vp, i32, i32, vp, vp, vp]
    if hasattr(L, "nbx_tidal"):  # likewise for nbx_tidal.hip
        L.nbx_tidal.argtypes = [vp, i32, vp, vp, vp, vp]
        L.nbx_ensemble_tidal.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
        L.nbx_ragged_tidal.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
        L.nbx_tidal_bodies.argtypes = [vp, vp]
        L.nbx_ensemble_tidal_bodies.argtypes = [vp, i32, i32, vp]
        L.nbx_ragged_tidal_bodies.argtypes = [vp, i32, i32, vp]
    if hasattr(L, "nbx_clumps"):  # likewise for nbx_clumps.hip
        L.nbx_clumps.argtypes = [vp, vp, ctypes.POINTER(ClumpsOut)]
        L.nbx_ensemble_clumps.argtypes = [vp, i32, i32, vp, ctypes.POINTER(ClumpsOut)]
        L.nbx_ragged_clumps.argtypes = [vp, i32, i32, vp, ctypes.POINTER(ClumpsOut)]
    if hasattr(L, "nbx_nlist"):  # likewise for nbx_nlist.hip
        i64 = ctypes.c_int64
        L.nbx_nlist.argtypes = [vp, dbl, i64, vp, vp, vp, vp]
        L.nbx_ensemble_nlist.argtypes = [vp, i32, i32, dbl, i64, vp, vp, vp, vp]
        L.nbx_ragged_nlist.argtypes = [vp, i32, i32, dbl, i64, vp, vp, vp, vp]
    if hasattr(L, "nbx_jerk"):  # likewise for nbx_jerk.hip
        L.nbx_jerk.argtypes = [vp, ctypes.POINTER(JerkOut)]
        L.nbx_ensemble_jerk.argtypes = [vp, i32, i32, ctypes.POINTER(JerkOut)]
        L.nbx_ragged_jerk.argtypes = [vp, i32, i32, ctypes.POINTER(JerkOut)]
    if hasattr(L, "nbx_hermite_step"):  # likewise for nbx_hermite.hip
        for name in HERMITE_SYMBOLS:
            getattr(L, name).argtypes = [vp, dbl, i32, i32]
    if hasattr(L, "nbx_advance"):  # likewise for nbx_advance.hip
        for name in ADVANCE_SYMBOLS[:3]:
            getattr(L, name).argtypes = [vp, dbl, dbl, i32, dbl, i32, i32]
        L.nbx_clock.argtypes = [vp, ctypes.POINTER(Clock)]
        L.nbx_ensemble_clock.argtypes = [vp, i32, i32, ctypes.POINTER(Clock)]
        L.nbx_ragged_clock.argtypes = [vp, i32, i32, ctypes.POINTER(Clock)]
    _lib = L
    return L


def _check(rc, where):
    if rc != NBX_OK:
        raise NbxError(rc, where, load().nbx_last_error().decode(errors="replace"))


def _dtype(precision):
    if precision == 32:
        return np.float32
    if precision == 64:
        return np.float64
    raise NbxError(NBX_ERR_ARG, "precision", "must be 32 or 64")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


DT = float(np.float32(0.1))  # (float)0.1 widened: the reference's _tstep (ver7/GSimulation.cpp:30)

FIELDS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")


def initial_conditions(n, precision=32):
    """Seed-42 particles of ver7/GSimulation.cpp:45-94 as a dict of seven arrays."""
    L = load()
    dt = _dtype(precision)
    s = {f: np.zeros(max(n, 0), dtype=dt) for f in FIELDS}
    _check(L.nbx_ic_pos(n, precision, _ptr(s["pos_x"]), _ptr(s["pos_y"]), _ptr(s["pos_z"])), "nbx_ic_pos")
    _check(L.nbx_ic_vel(n, precision, _ptr(s["vel_x"]), _ptr(s["vel_y"]), _ptr(s["vel_z"])), "nbx_ic_vel")
    _check(L.nbx_ic_mass(n, precision, _ptr(s["mass"])), "nbx_ic_mass")
    return s


def _opts(opts):
    """An nbx_opts at its defaults (device -1: the current one) with the keyword options written over them."""
    o = Opts()
    o.struct_size = ctypes.sizeof(Opts)
    o.device = -1
    for k, v in opts.items():
        if not hasattr(o, k):
            raise TypeError("unknown nbx_opts field %r" % k)
        setattr(o, k, v)
    return o


class _Handle:
    """A handle of the library and the entry point that destroys it: closed by close(), on leaving a `with` block, or with the
    Python object.  A subclass names the entry point in _destroy and creates the handle into self._h."""
    _destroy = None

    def _new_handle(self):
        self._L = load()
        self._h = ctypes.c_void_p()

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _need(L, where):
    if not hasattr(L, where):
        raise NbxError(NBX_ERR_STATE, where, "%s was built without %s" % (LIB_PATH, where))


def _neighbour_arrays(shape, dtype, radius):
    """The three result arrays of a *_neighbours call; within is None -- a NULL pointer to the library -- without a radius."""
    return {"index": np.zeros(shape, dtype=np.int32), "r2": np.zeros(shape, dtype=dtype),
            "within": None if radius is None else np.zeros(shape, dtype=np.int32)}


def _knn_arrays(rows, k, dtype):
    """The two result arrays of a *_knn call, `rows` rows of k (at least one element each: _ptr wants an address)."""
    size = max(rows * min(max(int(k), 0), KNN_MAX), 1)  # a k the library refuses needs no room
    return {"index": np.zeros(size, dtype=np.int32), "r2": np.zeros(size, dtype=dtype)}


def _fof_arrays(bodies, systems):
    """The four result arrays of a *_fof call (at least one element each: _ptr wants an address): label and size per body,
    {groups, largest} per system as an (systems, 2) int32 array -- nbx_fof_info_t's layout -- and the scalar passes."""
    return [np.zeros(max(bodies, 1), dtype=np.int32), np.zeros(max(bodies, 1), dtype=np.int32),
            np.zeros((max(systems, 1), 2), dtype=np.int32), np.zeros(1, dtype=np.int32)]


def _nlist(call, bodies, dtype, radius, capacity):
    """The two-call protocol of a *_nlist entry point: call(radius, capacity, offsets, index, r2, total) raises on a status other
    than NBX_OK.  capacity None: NLIST_FIRST_GUESS entries per body first, then the exact total if that was too small.  An explicit
    capacity is one call; where the lists do not fit it, "index" and "r2" are None and "total" says what they need."""
    offsets = np.zeros(max(bodies, 0) + 1, dtype=np.int64)
    total = np.zeros(1, dtype=np.int64)
    tries = [min(NLIST_FIRST_GUESS * max(bodies, 0), NLIST_MAX_CAPACITY), None] if capacity is None else [int(capacity)]
    for cap in tries:
        cap = int(total[0]) if cap is None else cap
        index = np.zeros(max(cap, 1), dtype=np.int32)  # at least one element each: _ptr wants an address
        r2 = np.zeros(max(cap, 1), dtype=dtype)
        call(radius, cap, _ptr(offsets), _ptr(index) if cap > 0 else None, _ptr(r2) if cap > 0 else None, _ptr(total))
        t = int(total[0])
        if t <= cap:
            return {"offsets": offsets, "index": index[:t].copy() if 2 * t < index.size else index[:t],
                    "r2": r2[:t].copy() if 2 * t < r2.size else r2[:t], "total": t}
    return {"offsets": offsets, "index": None, "r2": None, "total": int(total[0])}


def nlist_pairs(nl, n=None):
    """The unique pairs of an nlist() result: (pairs, r2), pairs a (k, 2) int64 array of (i, j), i < j, in the lists' order (by i,
    then by j), r2 their softened squared distances.  Every pair is in two lists with the same r2 bits; this keeps the one in
    the lower body's.  n None: the result of a Context.  n an int: of an Ensemble of n bodies per member; n a sequence of sizes:
    of a Ragged range of those members -- then one (pairs, r2) per member, i and j member-local."""
    offsets = np.asarray(nl["offsets"], dtype=np.int64)
    if nl["index"] is None or nl["r2"] is None:
        raise NbxError(NBX_ERR_ARG, "nlist_pairs", "the lists of this result were not filled (total exceeds the capacity)")
    bodies = offsets.shape[0] - 1
    if n is None:
        sizes = [bodies]
    elif np.ndim(n) == 0:
        if int(n) <= 0 or bodies % int(n):
            raise NbxError(NBX_ERR_ARG, "nlist_pairs", "the result's bodies are no multiple of n")
        sizes = [int(n)] * (bodies // int(n))
    else:
        sizes = [int(v) for v in n]
        if sum(sizes) != bodies:
            raise NbxError(NBX_ERR_ARG, "nlist_pairs", "the sizes do not add up to the result's bodies")
    at = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = []
    for m, size in enumerate(sizes):
        lo, hi = int(offsets[at[m]]), int(offsets[at[m + 1]])
        i = np.repeat(np.arange(size, dtype=np.int64), np.diff(offsets[at[m]:at[m + 1] + 1]))
        j = np.asarray(nl["index"][lo:hi], dtype=np.int64)
        keep = i < j
        out.append((np.stack([i[keep], j[keep]], axis=1).reshape(-1, 2), np.asarray(nl["r2"][lo:hi])[keep]))
    return out[0] if n is None else out


def _tidal_arrays(shape, dtype):
    """(the six result arrays of a *_tidal call by key, the void* t[6] that points at them)."""
    out = {k: np.zeros(shape, dtype=dtype) for k in TIDAL_KEYS}
    return out, (ctypes.c_void_p * 6)(*[out[k].ctypes.data for k in TIDAL_KEYS])


def tidal_matrix(res):
    """The symmetric (..., 3, 3) tidal tensors, in fp64, of a result of tidal() or tidal_bodies(): a dict of the six TIDAL_KEYS
    arrays of one shape."""
    c = [np.asarray(res[k], dtype=np.float64) for k in TIDAL_KEYS]
    return np.stack([np.stack([c[0], c[1], c[2]], axis=-1), np.stack([c[1], c[3], c[4]], axis=-1),
                     np.stack([c[2], c[4], c[5]], axis=-1)], axis=-2)


def tidal_radius(res, gm):
    """(gm / lambda_max)^(1/3), in fp64, lambda_max the largest eigenvalue of every tensor of `res` -- the strongest stretching
    -- and gm = G M of the object whose tidal radius is asked for (a scalar or an array of the tensors' shape); inf where
    lambda_max <= 0, i.e. where the field compresses along every axis.  The object's own softening is ignored."""
    lam = np.linalg.eigvalsh(tidal_matrix(res))[..., -1]
    gm = np.broadcast_to(np.asarray(gm, dtype=np.float64), lam.shape)
    out = np.full(lam.shape, np.inf)
    pos = lam > 0
    out[pos] = np.cbrt(gm[pos] / lam[pos])
    return out


def _binaries_arrays(shape, dtype, bound):
    """The three result arrays of a *_binaries call; bound is None -- a NULL pointer to the library -- where it is not asked for."""
    return {"partner": np.zeros(shape, dtype=np.int32), "energy": np.zeros(shape, dtype=dtype),
            "bound": np.zeros(shape, dtype=np.int32) if bound else None}


def binary_catalogue(partner, energy, mass, x, y, z, vx, vy, vz):
    """The mutual bound pairs of one system from binaries()'s partner and energy and the bodies' masses, positions and
    velocities: the (i, j), i < j, with partner[i] == j, partner[j] == i and energy[i] < 0, and their Kepler elements in fp64,
    as {"i", "j": (k,) int64, "energy": the specific two-body energy |dv|^2 / 2 - G (m_i + m_j) / |dx|, "a": the semi-major axis
    -G (m_i + m_j) / (2 energy), "ecc": the eccentricity sqrt(1 + 2 energy h^2 / (G (m_i + m_j))^2) from the specific angular
    momentum h = |dx x dv|, "period": 2 pi sqrt(a^3 / (G (m_i + m_j))), "binding": the binding energy mu |energy|, mu = m_i m_j /
    (m_i + m_j)}, sorted by binding energy, descending (then by i).  The elements IGNORE THE SOFTENING: the pairs are chosen by
    the library's softened energy, their elements are those of the unsoftened two-body problem, evaluated here from the state
    (the softened energy is never below it, so a pair the library calls bound is bound here too); two bodies at one position
    give a = 0."""
    partner = np.asarray(partner, dtype=np.int64)
    energy = np.asarray(energy, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    p = np.stack([np.asarray(a, dtype=np.float64) for a in (x, y, z)], axis=-1)
    v = np.stack([np.asarray(a, dtype=np.float64) for a in (vx, vy, vz)], axis=-1)
    if partner.ndim != 1 or energy.shape != partner.shape or mass.shape != partner.shape or p.shape != partner.shape + (3,) or v.shape != p.shape:
        raise NbxError(NBX_ERR_ARG, "binary_catalogue", "expected partner, energy, mass, x, y, z, vx, vy and vz of one shape (n,)")
    idx = np.arange(partner.shape[0])
    ok = (partner > idx) & (partner[np.clip(partner, 0, None)] == idx) & (energy < 0.0)
    i, j = idx[ok], partner[ok]
    dx, dv = p[j] - p[i], v[j] - v[i]
    gm = GRAV * (mass[i] + mass[j])
    with np.errstate(invalid="ignore", divide="ignore"):
        e = 0.5 * (dv * dv).sum(axis=1) - gm / np.sqrt((dx * dx).sum(axis=1))
        a = -gm / (2.0 * e)
        h = np.cross(dx, dv)
        ecc = np.sqrt(np.maximum(1.0 + 2.0 * e * (h * h).sum(axis=1) / (gm * gm), 0.0))
        period = 2.0 * np.pi * np.sqrt(a * a * a / gm)
        binding = mass[i] * mass[j] / (mass[i] + mass[j]) * np.abs(e)
    order = np.lexsort((i, -binding))
    return {"i": i[order], "j": j[order], "energy": e[order], "a": a[order], "ecc": ecc[order], "period": period[order],
            "binding": binding[order]}


def _clumps_arrays(shape, dtype):
    """(the ten result arrays of a *_clumps call by key, the nbx_clumps_out_t that points at them)."""
    out = {k: np.zeros(shape, dtype=np.int32 if k == "members" else dtype) for k in CLUMPS_KEYS}
    a = [out[k].ctypes.data for k in CLUMPS_KEYS]
    return out, ClumpsOut(a[0], a[1], (ctypes.c_void_p * 3)(*a[2:5]), (ctypes.c_void_p * 3)(*a[5:8]), a[8], a[9])


def _clumps_label(label, shape):
    """The caller's labels as a contiguous int32 array of `shape` (at least one element: an address is wanted)."""
    lab = np.asarray(label)
    if lab.shape != shape or lab.dtype.kind not in "iu" or (lab.size and (lab.min() < -2 ** 31 or lab.max() > 2 ** 31 - 1)):
        raise NbxError(NBX_ERR_ARG, "label", "expected integers that fit int32, of shape %r, got %s %r" % (shape, lab.dtype, lab.shape))
    lab = np.ascontiguousarray(lab, dtype=np.int32).reshape(-1)
    return lab if lab.size else np.zeros(1, dtype=np.int32)


def clump_catalogue(label, result, mass, min_members=2):
    """The clumps of one system from the labels given to clumps(), its result and the bodies' masses, in fp64: for every label
    >= 0 with at least `min_members` bodies one row of {"label", "members": (g,) int64, "gm": (g,), "centre", "velocity": (g, 3)
    -- the values the clump's first member returned; every member returns the same bits --, "kinetic": sum m_i |v_i - V|^2 / 2
    in the clump's own frame (from energy - phi), "potential": sum m_i phi_i / 2, "virial": 2 kinetic / |potential| (inf where
    the potential is 0), "bound": (g,) int64, the members with energy < 0}, ordered by (-members, label)."""
    label = np.asarray(label, dtype=np.int64)
    mass = np.asarray(mass, dtype=np.float64)
    r = {k: np.asarray(result[k], dtype=np.int64 if k == "members" else np.float64) for k in CLUMPS_KEYS}
    if label.ndim != 1 or mass.shape != label.shape or any(v.shape != label.shape for v in r.values()):
        raise NbxError(NBX_ERR_ARG, "clump_catalogue", "expected label, mass and the ten arrays of a clumps() result of one shape (n,)")
    at = np.nonzero(label >= 0)[0]
    names, first, inverse, members = np.unique(label[at], return_index=True, return_inverse=True, return_counts=True)
    g = len(names)
    kinetic = np.bincount(inverse, weights=mass[at] * (r["energy"][at] - r["phi"][at]), minlength=g)
    potential = 0.5 * np.bincount(inverse, weights=mass[at] * r["phi"][at], minlength=g)
    bound = np.bincount(inverse, weights=(r["energy"][at] < 0.0).astype(np.float64), minlength=g).astype(np.int64)
    keep = np.nonzero(members >= min_members)[0]
    keep = keep[np.lexsort((names[keep], -members[keep]))]
    lead = at[first[keep]] if g else np.zeros(0, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        virial = np.where(potential[keep] != 0.0, 2.0 * kinetic[keep] / np.abs(potential[keep]), np.inf)
    return {"label": names[keep].astype(np.int64), "members": members[keep].astype(np.int64), "gm": r["gm"][lead],
            "centre": np.stack([r["centre_" + a][lead] for a in "xyz"], axis=1),
            "velocity": np.stack([r["velocity_" + a][lead] for a in "xyz"], axis=1),
            "kinetic": kinetic[keep], "potential": potential[keep], "virial": virial, "bound": bound[keep]}


def unbind(obj, label, max_iter=32):
    """The unbinding iteration on a Context or an Ensemble: obj.clumps(label), then label = -1 wherever energy >= 0 (a clump of
    one body has energy 0 and leaves too), repeated until a call changes nothing or max_iter calls have been made.  Returns
    (label, result, iterations): the final labels (int32, the shape given), the result of the last call and the number of calls.
    Where the iteration ended by itself the result is that of the final labels."""
    if not isinstance(obj, (Context, Ensemble)):
        raise NbxError(NBX_ERR_ARG, "unbind", "expected a Context or an Ensemble")
    label = np.array(label, dtype=np.int32)
    result, iterations = None, 0
    while iterations < max_iter:
        result = obj.clumps(label)
        iterations += 1
        leave = (label >= 0) & (result["energy"] >= 0)
        if not leave.any():
            break
        label[leave] = -1
    return label, result, iterations


def _jerk_arrays(shape, dtype):
    """(the six result arrays of a *_jerk call by key, the nbx_jerk_out_t that points at them)."""
    out = {k: np.zeros(shape, dtype=dtype) for k in JERK_KEYS}
    a = [out[k].ctypes.data for k in JERK_KEYS]
    return out, JerkOut((ctypes.c_void_p * 3)(*a[:3]), (ctypes.c_void_p * 3)(*a[3:]))


def jerk_dt(result, eta):
    """The first-order time-step criterion per body from one jerk() result (a dict of the six JERK_KEYS arrays, any shape):
    eta |a| / |adot| in fp64, +inf where |adot| = 0."""
    r = {k: np.asarray(result[k], dtype=np.float64) for k in JERK_KEYS}
    a = np.sqrt(r["acc_x"] ** 2 + r["acc_y"] ** 2 + r["acc_z"] ** 2)
    j = np.sqrt(r["jerk_x"] ** 2 + r["jerk_y"] ** 2 + r["jerk_z"] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(j > 0.0, float(eta) * a / j, np.inf)


def _remember_mass(obj, first, masses):
    """upload() keeps the masses it was given, per member: the library returns positions and velocities only, and hermite()
    uploads states of its own."""
    obj._hermite_stale = True  # what a Hermite call kept belongs to the state before this upload (hermite_step, resume)
    obj._advance_stale = True  # and so do the clocks and the kept records of an advance call (advance, resume)
    if not hasattr(obj, "_mass"):
        obj._mass = {}
    for k, m in enumerate(masses):
        obj._mass[first + k] = np.array(m, dtype=obj.dtype)


def _hermite_io(obj):
    """(download, upload, jerk, masses) of the object as lists of per-system dicts (an ensemble: one dict of (members, n) arrays)."""
    if not isinstance(obj, (Context, Ensemble, Ragged)):
        raise NbxError(NBX_ERR_ARG, "hermite", "expected a Context, an Ensemble or a Ragged")
    members = 1 if isinstance(obj, Context) else obj.members
    kept = getattr(obj, "_mass", {})
    for k in range(members):
        if k not in kept:
            raise NbxError(NBX_ERR_STATE, "hermite", "member %d has not been uploaded through this object: its masses are not known" % k)
    if isinstance(obj, Ragged):
        return obj.download, obj.upload, obj.jerk, [kept[k] for k in range(members)]
    mass = kept[0] if isinstance(obj, Context) else np.stack([kept[k] for k in range(members)])
    return (lambda: [obj.download()]), (lambda s: obj.upload(s[0])), (lambda: [obj.jerk()]), [mass]


def hermite(obj, dt, nsteps):
    """nsteps fourth-order Hermite P(EC) steps of dt on a Context, an Ensemble or a Ragged, by host round trip over jerk():
    the state is downloaded once at the start and a and adot taken there; per step the host predicts
        xp = x + v dt + a dt^2/2 + adot dt^3/6,   vp = v + a dt + adot dt^2/2,
    uploads the predicted state, calls jerk() for a1, adot1 there and corrects
        v1 = v + (a + a1) dt/2 + (adot - adot1) dt^2/12,   x1 = x + (v + v1) dt/2 + (a - a1) dt^2/12
    in fp64; a1 and adot1 start the next step (no second evaluation), and the corrected state is uploaded after the last step.
    Cost: one upload and one read-back of O(n) per step, beside the jerk's pair work -- what a device-resident stepper would not
    pay.  The masses are those given to this object's upload().  steps_done does not count these steps: it is what it was.  The
    energies: as after any upload, the kinetic-energy partials belong to no state, so a step call of no steps reports 0 until a
    step or a kick has run; diagnostics() sees the corrected state.  Returns the corrected state, the list of per-system dicts
    uploaded last (fp64; one dict of (members, n) arrays for an ensemble); None where nsteps == 0."""
    download, upload, jerk, mass = _hermite_io(obj)
    if nsteps < 0:
        raise NbxError(NBX_ERR_ARG, "hermite", "nsteps is negative")
    if nsteps == 0:
        return None
    dt = float(dt)
    pos, vel = FIELDS[:3], FIELDS[3:6]
    acc, jrk = JERK_KEYS[:3], JERK_KEYS[3:]
    st = [{f: np.asarray(s[f], dtype=np.float64) for f in FIELDS[:6]} for s in download()]
    d0 = [{k: np.asarray(r[k], dtype=np.float64) for k in JERK_KEYS} for r in jerk()]
    for step in range(nsteps):
        pred = []
        for s, d, m in zip(st, d0, mass):
            p = {"mass": m}
            for x, v, a, j in zip(pos, vel, acc, jrk):
                p[x] = s[x] + dt * (s[v] + dt * (d[a] / 2.0 + dt * d[j] / 6.0))
                p[v] = s[v] + dt * (d[a] + dt * d[j] / 2.0)
            pred.append(p)
        upload(pred)
        d1 = [{k: np.asarray(r[k], dtype=np.float64) for k in JERK_KEYS} for r in jerk()]
        new = []
        for s, d, e in zip(st, d0, d1):
            c = {}
            for x, v, a, j in zip(pos, vel, acc, jrk):
                c[v] = s[v] + dt * ((d[a] + e[a]) / 2.0 + dt * (d[j] - e[j]) / 12.0)
                c[x] = s[x] + dt * ((s[v] + c[v]) / 2.0 + dt * (d[a] - e[a]) / 12.0)
            new.append(c)
        st, d0 = new, d1
    upload([dict(s, mass=m) for s, m in zip(st, mass)])
    return st


def fof_catalogue(label, mass, x, y, z, min_members=2):
    """The groups of one system from fof()'s label and the bodies' masses and positions, in fp64: for every group of at least
    `min_members` bodies its label, members, mass and centre of mass, as {"label": (g,) int64, "members": (g,) int64, "mass":
    (g,), "centre": (g, 3)}, ordered by (-members, label)."""
    label = np.asarray(label, dtype=np.int64)
    mass = np.asarray(mass, dtype=np.float64)
    p = np.stack([np.asarray(a, dtype=np.float64) for a in (x, y, z)], axis=1)
    if label.ndim != 1 or mass.shape != label.shape or p.shape != label.shape + (3,):
        raise NbxError(NBX_ERR_ARG, "fof_catalogue", "expected label, mass, x, y and z of one shape (n,)")
    names, inverse, members = np.unique(label, return_inverse=True, return_counts=True)
    total = np.bincount(inverse, weights=mass, minlength=len(names))
    moment = np.stack([np.bincount(inverse, weights=mass * p[:, a], minlength=len(names)) for a in range(3)], axis=1)
    keep = members >= min_members
    names, members, total, moment = names[keep], members[keep], total[keep], moment[keep]
    order = np.lexsort((names, -members))
    with np.errstate(invalid="ignore", divide="ignore"):
        centre = moment[order] / total[order][:, None]
    return {"label": names[order].astype(np.int64), "members": members[order].astype(np.int64), "mass": total[order], "centre": centre}


def local_density(knn, mass):
    """The local density estimator of Casertano & Hut from a knn() result of k >= 2 columns and the bodies' masses, in fp64:
    rho_i = (the masses of the first k - 1 neighbours, summed) / (4/3 pi d_k^3), d_k^2 = max(r2[i, k - 1] - eps^2, 0) the
    unsoftened squared distance to the k-th neighbour.  A row with fill -- a body with fewer than k partners -- gives 0, and so
    does a body whose k-th neighbour sits on it (d_k = 0)."""
    index = np.asarray(knn["index"])
    r2 = np.asarray(knn["r2"], dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    if index.ndim != 2 or index.shape != r2.shape or index.shape[1] < 2 or mass.shape != index.shape[:1]:
        raise NbxError(NBX_ERR_ARG, "local_density", "expected index and r2 of shape (n, k), k >= 2, and n masses")
    k = index.shape[1]
    full = (index >= 0).all(axis=1)
    d2 = np.maximum(np.where(full, r2[:, k - 1], np.inf) - EPS2, 0.0)
    inside = np.where(full[:, None], mass[np.clip(index[:, :k - 1], 0, None)], 0.0).sum(axis=1)
    rho = np.zeros(index.shape[0])
    ok = full & (d2 > 0.0)
    rho[ok] = inside[ok] / (4.0 / 3.0 * np.pi * d2[ok] ** 1.5)
    return rho


def density_centre(x, y, z, rho):
    """(centre[3], core_radius) of Casertano & Hut from positions and local_density()'s rho, in fp64:
    centre = sum rho_i x_i / sum rho_i,  core_radius = sqrt(sum rho_i^2 |x_i - centre|^2 / sum rho_i^2)."""
    p = np.stack([np.asarray(a, dtype=np.float64) for a in (x, y, z)], axis=1)
    rho = np.asarray(rho, dtype=np.float64)
    centre = (rho[:, None] * p).sum(axis=0) / rho.sum()
    d2 = ((p - centre) ** 2).sum(axis=1)
    return centre, float(np.sqrt((rho * rho * d2).sum() / (rho * rho).sum()))


def _batch_paircount(o, radii, first, count):
    """paircount() of an Ensemble or a Ragged."""
    _need(o._L, o._prefix + "_paircount")
    count = o.members - first if count is None else count
    r = _radii(radii)
    out = np.zeros((max(count, 0), r.shape[0]), dtype=np.uint64)
    o._call("paircount", first, count, r.shape[0], _ptr(r), _ptr(out) if out.size else None)
    return out


def _radii(radii):
    """The radii of a *_paircount call as the contiguous array of doubles the library reads."""
    return np.ascontiguousarray(np.atleast_1d(np.asarray(radii, dtype=np.float64)).reshape(-1))


def shell_counts(counts):
    """The pair-separation histogram of paircount()'s result for ASCENDING radii: element k is the number of pairs in the shell
    (radii[k - 1], radii[k]], element 0 the pairs within radii[0]; along the last axis, same shape and dtype."""
    counts = np.asarray(counts)
    return np.diff(counts, axis=-1, prepend=counts.dtype.type(0))


def mutual_pairs(index):
    """The (i, j), i < j, with index[i] == j and index[j] == i -- mutual nearest neighbours -- as a (k, 2) int array."""
    index = np.asarray(index)
    i = np.arange(index.shape[0])
    ok = (index > i) & (index[np.clip(index, 0, None)] == i)
    return np.stack([i[ok], index[ok]], axis=1).astype(np.int64).reshape(-1, 2)


class _Leapfrog:
    """leapfrog() over a class's own kick() and step() (include/nbx_kick.h)."""

    def leapfrog(self, nsteps, dt=DT, kenergy=True):
        """kick(-dt/2); step(nsteps, dt); kick(+dt/2): kick-drift-kick leapfrog -- second order and time reversible, its steps
        the plain step launches.  Positions and velocities are at the same time afterwards; the kinetic energy, if asked for, is
        that of the final velocities."""
        self.kick(-0.5 * dt)
        self.step(nsteps, dt, kenergy=False)
        return self.kick(0.5 * dt, kenergy)


class _Tracers:
    """The resident tracers of include/nbx_tracers.h over a class's own _tracers_call(name, *args) -- the C-ABI call
    <prefix>_tracers_<name> on its handle -- and _tracers_range(first, count) -> (leading range arguments, array shape before m)."""

    def tracers_upload(self, points, velocities, first=0):
        """<prefix>_tracers_upload: points = (px, py, pz) and velocities = (vx, vy, vz), six arrays of one shape -- (m,) for a
        context, (count, m) for members first, first + 1, ... of a batch object (row k the tracers of member first + k).  Replaces
        the set; m == 0 removes it.  The first upload fixes m for a batch object.  Synchronises."""
        a = [np.ascontiguousarray(x, dtype=self.dtype) for x in tuple(points) + tuple(velocities)]
        lead, shape = self._tracers_range(first, a[0].shape[0] if a[0].ndim == 2 else None)
        if len(a) != 6 or a[0].ndim != len(shape) + 1 or any(x.shape != a[0].shape for x in a):
            raise NbxError(NBX_ERR_ARG, "array", "expected six arrays of one shape %s, got %r" % (shape + ("m",), [x.shape for x in a]))
        self._tracers_call("upload", *lead, a[0].shape[-1], *[_ptr(x) for x in a])

    def tracers_download(self, first=0, count=None):
        """<prefix>_tracers_download: {"pos_x", ..., "vel_z"}, arrays (m,) for a context, (count, m) for members
        [first, first + count) of a batch object (default: all from `first`).  Synchronises."""
        lead, shape = self._tracers_range(first, count, default=True)
        m = self.tracers_count()
        out = {f: np.zeros(shape + (m,), dtype=self.dtype) for f in FIELDS[:6]}
        self._tracers_call("download", *lead, *[_ptr(out[f]) for f in FIELDS[:6]])
        return out

    def tracers_count(self):
        """<prefix>_tracers_count: tracers per system (0: none)."""
        m = ctypes.c_int32(0)
        self._tracers_call("count", ctypes.byref(m))
        return m.value

    def tracers_step(self, nsteps, dt=DT, kenergy=True):
        """<prefix>_tracers_step: nsteps steps of the bodies -- the bits step() gives -- and of every tracer, each tracer step in
        the field of the bodies before their step; the bodies' kinetic energy after the last one if asked for (synchronises)."""
        batch = hasattr(self, "members")
        ke = (np.zeros(self.members, dtype=np.float64) if batch else np.zeros(1, dtype=np.float64)) if kenergy else None
        self._tracers_call("step", dt, nsteps, _ptr(ke))
        return None if ke is None else ke if batch else float(ke[0])

    def tracers_kick(self, h):
        """<prefix>_tracers_kick: w += a(p) * h for every tracer at the bodies' current positions; tracer positions and the
        bodies untouched.  Does not synchronise."""
        self._tracers_call("kick", h)

    def tracers_leapfrog(self, nsteps, dt=DT, kenergy=True):
        """Kick-drift-kick leapfrog of the joint system: kick(-dt/2) on bodies and tracers, tracers_step(nsteps, dt), kick(+dt/2)
        on both.  The bodies' kinetic energy of the final velocities if asked for."""
        self.kick(-0.5 * dt)
        self.tracers_kick(-0.5 * dt)
        self.tracers_step(nsteps, dt, kenergy=False)
        self.tracers_kick(0.5 * dt)
        return self.kick(0.5 * dt, kenergy)


class _Hermite:
    """hermite_step() over the C-ABI call a class names in _hermite (include/nbx_hermite.h)."""

    def hermite_step(self, dt, nsteps=1, resume=False):
        """<prefix>_hermite_step: nsteps fourth-order Hermite P(EC) steps of dt of every body (of every member of a batch object)
        on the device -- hermite()'s scheme without its round trip: two launches a step, nothing read back, no synchronisation.
        resume=False evaluates the acceleration and its time derivative at the resident state first (two more launches);
        resume=True continues from what the previous hermite_step() on this object kept, so that (dt, a) then (dt, b, resume=True)
        is (dt, a + b) bit for bit -- the caller promises that no upload, step, kick, commit or local step came between (analysis
        calls may).  The library refuses (NBX_ERR_STATE) what it sees of a broken promise -- no previous call, a step, a kick --
        and this object refuses an upload made through it, which the library cannot see.  steps_done does not count these steps,
        tracers do not move, and as after an upload a step call of no steps reports 0 until a step or a kick has run."""
        _need(self._L, self._hermite)
        if resume and getattr(self, "_hermite_stale", False) and getattr(self, "_hermite_kept", False):
            raise NbxError(NBX_ERR_STATE, self._hermite, "%s: resume after an upload (what the previous Hermite call kept belongs to "
                           "the state before it)" % self._hermite)
        _check(getattr(self._L, self._hermite)(self._h, dt, nsteps, 1 if resume else 0), self._hermite)
        if nsteps > 0:
            self._hermite_stale, self._hermite_kept = False, True


class _Advance:
    """advance() and clock() over the C-ABI calls a class names in _advance and _clock (include/nbx_advance.h)."""

    def advance(self, t_end, dt_cap, eta=0.125, levels=20, max_steps=32, resume=False):
        """<prefix>_advance: up to max_steps fourth-order Hermite P(EC) steps of every system -- the context, or each member of a
        batch object -- towards t_end, every system with a clock of its own and a step it chooses itself on the device: a power
        of two in [dt_cap * 2**-levels, dt_cap], eta * sqrt(q) rounded down, q the smallest of the bodies' step criteria.  dt_cap
        is a power of two and t_end a whole multiple of it, so every system lands on t_end exactly and then stops.  Three launches
        a step, nothing read back, no synchronisation: call advance(max_steps = a few dozen), then clock(), until every system
        is done.  resume=False starts the clocks at t = 0 and evaluates at the resident state first (also with max_steps=0, so
        that clock()["dt_next"] can be asked for before the first step); resume=True continues -- the caller promises that no
        upload, step, kick, commit, local step or hermite_step() came between (analysis calls may); dt_cap and levels must be
        the previous call's, eta may change, t_end may grow.  The library refuses (NBX_ERR_STATE) what it sees of a broken
        promise, and this object refuses an upload made through it.  A step of size h leaves the bits hermite_step(h) leaves;
        steps_done does not count these steps and tracers do not move."""
        _need(self._L, self._advance)
        if resume and getattr(self, "_advance_stale", False) and getattr(self, "_advance_kept", False):
            raise NbxError(NBX_ERR_STATE, self._advance, "%s: resume after an upload (the clocks and what the previous advance call "
                           "kept belong to the state before it)" % self._advance)
        _check(getattr(self._L, self._advance)(self._h, t_end, dt_cap, levels, eta, max_steps, 1 if resume else 0), self._advance)
        if not resume:
            self._advance_stale, self._advance_kept = False, True

    def clock(self, first=0, count=None):
        """<prefix>_clock: {"n", "t", "dt_last", "dt_next", "steps", "floor_steps", "done"} of the context, or one such dict per
        member of [first, first + count) of a batch object (default: all from `first`).  Synchronises once."""
        _need(self._L, self._clock)
        if not hasattr(self, "members"):
            if first != 0 or count is not None:
                raise NbxError(NBX_ERR_ARG, self._clock, "a context has one clock: no member range")
            c = Clock()
            c.struct_size = ctypes.sizeof(Clock)
            _check(getattr(self._L, self._clock)(self._h, ctypes.byref(c)), self._clock)
            return c.asdict()
        count = self.members - first if count is None else count
        c = (Clock * max(count, 1))()
        for k in range(max(count, 0)):
            c[k].struct_size = ctypes.sizeof(Clock)
        _check(getattr(self._L, self._clock)(self._h, first, count, c), self._clock)
        return [c[k].asdict() for k in range(max(count, 0))]


def suggest_dt(ts, eta):
    """eta / sqrt(rate) with rate the largest approach_rate2 or freefall_rate2 of `ts` -- one dict of timescale() or a list of
    them (the members of a batch object: the step all of them can take) -- or inf where every rate is 0."""
    entries = [ts] if isinstance(ts, dict) else list(ts)
    rate = max([max(t["approach_rate2"], t["freefall_rate2"]) for t in entries], default=0.0)
    return eta / math.sqrt(rate) if rate > 0.0 else math.inf


class _Adaptive:
    """adaptive() over a class's own timescale() and step() (include/nbx_timescale.h)."""

    def adaptive(self, t_end, eta, dt_max, max_steps=100000):
        """Plain steps from t = 0 to t_end, each of dt = min(dt_max, suggest_dt(self.timescale(), eta), t_end - t): one
        timescale call and one step call per turn, every member of a batch object taking the same dt, the smallest any member
        asks for.  Returns (t, steps, dts) with t == t_end; RuntimeError if max_steps turns do not get there."""
        t, dts = 0.0, []
        while t < t_end:
            if len(dts) >= max_steps:
                raise RuntimeError("adaptive: t = %r of %r after max_steps = %d steps" % (t, t_end, max_steps))
            dt = min(dt_max, suggest_dt(self.timescale(), eta), t_end - t)
            self.step(1, dt, kenergy=False)
            dts.append(dt)
            t = t_end if dt == t_end - t else t + dt
        return t, len(dts), dts


class Context(_Handle, _Leapfrog, _Adaptive, _Tracers, _Hermite, _Advance):
    """One nbx_ctx.  Keyword options are the nbx_opts fields."""
    _destroy = "nbx_destroy"
    _hermite = "nbx_hermite_step"
    _advance = "nbx_advance"
    _clock = "nbx_clock"

    def __init__(self, n, precision=32, **opts):
        self._new_handle()
        self.n = int(n)
        self.precision = int(precision)
        o = _opts(opts)
        _check(self._L.nbx_create(ctypes.byref(self._h), self.n, self.precision, ctypes.byref(o)), "nbx_create")
        self.dtype = _dtype(self.precision)

    def _arr(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.shape != (self.n,):
            raise NbxError(NBX_ERR_ARG, "array", "expected shape (%d,), got %r" % (self.n, a.shape))
        return a

    def upload(self, state):
        arrs = [self._arr(state[f]) for f in FIELDS]
        _check(self._L.nbx_upload(self._h, *[_ptr(a) for a in arrs]), "nbx_upload")
        _remember_mass(self, 0, [arrs[6]])

    def step(self, nsteps, dt=DT, kenergy=True):
        ke = ctypes.c_double(0.0)
        _check(self._L.nbx_step(self._h, dt, nsteps, ctypes.byref(ke) if kenergy else None), "nbx_step")
        return ke.value if kenergy else None

    def step_trace(self, nsteps, dt=DT):
        ke = np.zeros(max(nsteps, 1), dtype=np.float64)
        _check(self._L.nbx_step_trace(self._h, dt, nsteps, _ptr(ke)), "nbx_step_trace")
        return ke[:nsteps]

    def kick(self, h, kenergy=False):
        """nbx_kick: v += a(x) * h for the owned bodies at the current positions; positions untouched.  The kinetic energy of the
        kicked velocities if asked for (synchronises)."""
        _need(self._L, "nbx_kick")
        ke = ctypes.c_double(0.0)
        _check(self._L.nbx_kick(self._h, h, ctypes.byref(ke) if kenergy else None), "nbx_kick")
        return ke.value if kenergy else None

    def timescale(self):
        """nbx_timescale: approach_rate2, freefall_rate2 and min_r2 over all pairs of the current state (plus n and
        steps_done); suggest_dt() turns them into a step.  Synchronises."""
        _need(self._L, "nbx_timescale")
        t = Timescale()
        t.struct_size = ctypes.sizeof(Timescale)
        _check(self._L.nbx_timescale(self._h, ctypes.byref(t)), "nbx_timescale")
        return t.asdict()

    def field(self, px, py, pz):
        """nbx_field: the acceleration and the potential of the resident bodies at the m points (px, py, pz) -- every body
        counts, a point is not a body -- as {"acc_x", "acc_y", "acc_z", "phi"}, arrays of m.  Synchronises."""
        _need(self._L, "nbx_field")
        p = [np.ascontiguousarray(a, dtype=self.dtype) for a in (px, py, pz)]
        if p[0].ndim != 1 or any(a.shape != p[0].shape for a in p):
            raise NbxError(NBX_ERR_ARG, "array", "expected three arrays of one shape (m,), got %r" % ([a.shape for a in p],))
        m = p[0].shape[0]
        out = {k: np.zeros(m, dtype=self.dtype) for k in FIELD_KEYS}
        _check(self._L.nbx_field(self._h, m, *[_ptr(a) for a in p], *[_ptr(out[k]) for k in FIELD_KEYS]), "nbx_field")
        return out

    def neighbours(self, radius=None):
        """nbx_neighbours: for every body its nearest neighbour, the softened squared distance to it and the number of bodies
        within `radius`, as {"index", "r2", "within"}, arrays of n (all n bodies, also for a sliced context).  within is None
        when radius is None: the count is then neither asked for nor paid for.  Synchronises."""
        _need(self._L, "nbx_neighbours")
        out = _neighbour_arrays((self.n,), self.dtype, radius)
        _check(self._L.nbx_neighbours(self._h, 0.0 if radius is None else radius, *[_ptr(out[k]) for k in NEIGHBOUR_KEYS]), "nbx_neighbours")
        return out

    def knn(self, k):
        """nbx_knn: for every body its k nearest neighbours, ascending in (r2, index), and the softened squared distances to
        them, as {"index": (n, k) int32, "r2": (n, k)} (all n bodies, also for a sliced context); entries a body has no partner
        for are index -1, r2 +inf.  1 <= k <= KNN_MAX.  Synchronises."""
        _need(self._L, "nbx_knn")
        flat = _knn_arrays(self.n, k, self.dtype)
        _check(self._L.nbx_knn(self._h, k, *[_ptr(flat[key]) for key in KNN_KEYS]), "nbx_knn")
        return {key: flat[key][:self.n * k].reshape(self.n, k) for key in KNN_KEYS}

    def binaries(self, bound=True):
        """nbx_binaries: for every body its most bound partner, the specific two-body energy of that pair and the number of
        bodies it is bound to, as {"partner", "energy", "bound"}, arrays of n.  bound is None when bound=False: the count is then
        neither asked for nor paid for.  A sliced context is refused.  Synchronises."""
        _need(self._L, "nbx_binaries")
        out = _binaries_arrays((self.n,), self.dtype, bound)
        _check(self._L.nbx_binaries(self._h, *[_ptr(out[k]) for k in BINARIES_KEYS]), "nbx_binaries")
        return out

    def clumps(self, label):
        """nbx_clumps: under the int32 labels `label` (n,) -- any value >= 0 names a clump, a negative one means "in no clump" --
        for every body the members, G m, centre and mean velocity of its clump, the potential of the clump's other members at
        the body and its specific energy in the clump's frame, as the ten CLUMPS_KEYS arrays of n.  A sliced context is refused.
        Synchronises."""
        _need(self._L, "nbx_clumps")
        lab = _clumps_label(label, (self.n,))
        out, a = _clumps_arrays((self.n,), self.dtype)
        _check(self._L.nbx_clumps(self._h, _ptr(lab), ctypes.byref(a)), "nbx_clumps")
        return out

    def jerk(self):
        """nbx_jerk: the acceleration of every body and its time derivative at the current positions and velocities, as the six
        JERK_KEYS arrays of n; acc is bit for bit field()'s at the bodies' own positions.  A sliced context is refused.
        Synchronises."""
        _need(self._L, "nbx_jerk")
        out, a = _jerk_arrays((self.n,), self.dtype)
        _check(self._L.nbx_jerk(self._h, ctypes.byref(a)), "nbx_jerk")
        return out

    def tidal(self, px, py, pz):
        """nbx_tidal: the tidal tensor of the resident bodies at the m points (px, py, pz) -- every body counts, a point is not a
        body -- as {"t_xx", "t_xy", "t_xz", "t_yy", "t_yz", "t_zz"}, arrays of m.  Synchronises."""
        _need(self._L, "nbx_tidal")
        p = [np.ascontiguousarray(a, dtype=self.dtype) for a in (px, py, pz)]
        if p[0].ndim != 1 or any(a.shape != p[0].shape for a in p):
            raise NbxError(NBX_ERR_ARG, "array", "expected three arrays of one shape (m,), got %r" % ([a.shape for a in p],))
        m = p[0].shape[0]
        out, t = _tidal_arrays(m, self.dtype)
        _check(self._L.nbx_tidal(self._h, m, *[_ptr(a) for a in p], t), "nbx_tidal")
        return out

    def tidal_bodies(self):
        """nbx_tidal_bodies: the tidal tensor at every body, the body's own term never formed, as the six TIDAL_KEYS arrays of n
        (all n bodies, also for a sliced context).  Synchronises."""
        _need(self._L, "nbx_tidal_bodies")
        out, t = _tidal_arrays(self.n, self.dtype)
        _check(self._L.nbx_tidal_bodies(self._h, t), "nbx_tidal_bodies")
        return out

    def fof(self, radius):
        """nbx_fof: the friends-of-friends groups at linking length `radius`, as {"label": (n,) int32 -- the lowest index of the
        body's group --, "size": (n,) int32, "groups", "largest", "passes"} (all n bodies, also for a sliced context).
        Synchronises once per pass."""
        _need(self._L, "nbx_fof")
        label, size, info, passes = _fof_arrays(self.n, 1)
        _check(self._L.nbx_fof(self._h, radius, _ptr(label), _ptr(size), _ptr(info), _ptr(passes)), "nbx_fof")
        return {"label": label[:self.n], "size": size[:self.n], "groups": int(info[0, 0]), "largest": int(info[0, 1]), "passes": int(passes[0])}

    def nlist(self, radius, capacity=None):
        """nbx_nlist: for every body the indices of all bodies within `radius` (r2 <= h2 = fma(r, r, eps^2)), ascending, and their
        r2, as {"offsets": (n + 1,) int64, "index": (total,) int32, "r2": (total,), "total"}: the list of body i is
        index[offsets[i]:offsets[i + 1]].  capacity None: two calls at most; an int: one call, index and r2 None where
        total exceeds it; 0: the counting call.  Synchronises once per pass."""
        _need(self._L, "nbx_nlist")
        return _nlist(lambda *a: _check(self._L.nbx_nlist(self._h, *a), "nbx_nlist"), self.n, self.dtype, radius, capacity)

    def paircount(self, radii):
        """nbx_paircount: the number of pairs i < j with r2(i, j) <= h2 for each of `radii` (any order, at most 256), a
        np.uint64 array of len(radii) -- of all n bodies, also for a sliced context; one pass over the pairs per 16 radii.
        Synchronises."""
        _need(self._L, "nbx_paircount")
        r = _radii(radii)
        out = np.zeros(r.shape[0], dtype=np.uint64)
        _check(self._L.nbx_paircount(self._h, r.shape[0], _ptr(r), _ptr(out)), "nbx_paircount")
        return out

    def _tracers_call(self, name, *args):
        where = "nbx_tracers_" + name
        _need(self._L, where)
        _check(getattr(self._L, where)(self._h, *args), where)

    def _tracers_range(self, first, count, default=False):
        if first != 0 or count is not None:
            raise NbxError(NBX_ERR_ARG, "tracers", "a context has one system: no member range")
        return (), ()

    def step_local(self, dt=DT):
        _check(self._L.nbx_step_local(self._h, dt), "nbx_step_local")

    def exchange_buffer(self):
        p = ctypes.c_void_p()
        tot, off, own = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _check(self._L.nbx_exchange_buffer(self._h, ctypes.byref(p), ctypes.byref(tot), ctypes.byref(off),
                                           ctypes.byref(own)), "nbx_exchange_buffer")
        return p.value, tot.value, off.value, own.value

    def commit(self):
        _check(self._L.nbx_commit(self._h), "nbx_commit")

    def kenergy_partial(self):
        s = ctypes.c_double(0.0)
        _check(self._L.nbx_kenergy_partial(self._h, ctypes.byref(s)), "nbx_kenergy_partial")
        return s.value

    def accel(self):
        a = [np.zeros(self.n, dtype=self.dtype) for _ in range(3)]
        _check(self._L.nbx_accel(self._h, *[_ptr(x) for x in a]), "nbx_accel")
        return a

    def sync(self):
        _check(self._L.nbx_sync(self._h), "nbx_sync")

    def download(self):
        out = {f: np.zeros(self.n, dtype=self.dtype) for f in FIELDS[:6]}
        _check(self._L.nbx_download(self._h, *[_ptr(out[f]) for f in FIELDS[:6]]), "nbx_download")
        return out

    def profile(self, enable=True):
        _check(self._L.nbx_profile(self._h, 1 if enable else 0), "nbx_profile")

    def stats(self):
        s = Stats()
        _check(self._L.nbx_stats(self._h, ctypes.byref(s)), "nbx_stats")
        return s.asdict()

    def diagnostics(self):
        """nbx_diagnostics: this context's owned-slice partials (mass, kenergy, potential, momentum, mass_moment, i_count,
        steps_done) of the current state, plus etotal = kenergy + potential."""
        d = Diag()
        d.struct_size = ctypes.sizeof(Diag)
        _check(self._L.nbx_diagnostics(self._h, ctypes.byref(d)), "nbx_diagnostics")
        return d.asdict()


class _Batch(_Handle, _Leapfrog, _Adaptive, _Tracers, _Hermite, _Advance):
    """What Ensemble and Ragged share -- the library serves both from one host layer (csrc/nbx_batch.hpp), and every method here
    is the C-ABI call of that name under the class's prefix.  A subclass sets members and precision, calls _create, and adds
    upload and download, which differ in how the members' arrays are laid out."""
    _prefix = None   # "nbx_ensemble": <prefix>_create, <prefix>_step, ...
    _stats = None    # the ctypes mirror of <prefix>_stats_t
    _what = None     # the entry points, as the "was built without ..." error names them
    _hermite = property(lambda self: self._prefix + "_hermite_step")
    _advance = property(lambda self: self._prefix + "_advance")
    _clock = property(lambda self: self._prefix + "_clock")

    def _call(self, name, *args):
        where = "%s_%s" % (self._prefix, name)
        _check(getattr(self._L, where)(self._h, *args), where)

    def _create(self, opts, *args):
        """<prefix>_create(&handle, *args, &nbx_opts) on a library that has this kind's entry points."""
        self._new_handle()
        self._destroy = self._prefix + "_destroy"
        where = self._prefix + "_create"
        if not hasattr(self._L, where):
            raise NbxError(NBX_ERR_STATE, where, "%s was built without %s" % (LIB_PATH, self._what))
        o = _opts(opts)
        _check(getattr(self._L, where)(ctypes.byref(self._h), *args, ctypes.byref(o)), where)
        self.dtype = _dtype(self.precision)

    def step(self, nsteps, dt=DT, kenergy=True):
        """nsteps steps of every member; the kinetic energy of each member after the last one (array of `members`) if asked for."""
        ke = np.zeros(self.members, dtype=np.float64) if kenergy else None
        self._call("step", dt, nsteps, _ptr(ke))
        return ke

    def step_trace(self, nsteps, dt=DT):
        """The kinetic energy of every member after every step: array (nsteps, members)."""
        ke = np.zeros((max(nsteps, 1), self.members), dtype=np.float64)
        self._call("step_trace", dt, nsteps, _ptr(ke))
        return ke[:nsteps]

    def kick(self, h, kenergy=False):
        """<prefix>_kick: v += a(x) * h for every body of every member at the current positions, one launch; positions untouched.
        The kinetic energy of each member's kicked velocities (array of `members`) if asked for (synchronises)."""
        _need(self._L, self._prefix + "_kick")
        ke = np.zeros(self.members, dtype=np.float64) if kenergy else None
        self._call("kick", h, _ptr(ke))
        return ke

    def sync(self):
        self._call("sync")

    def profile(self, enable=True):
        self._call("profile", 1 if enable else 0)

    def stats(self):
        s = self._stats()
        s.struct_size = ctypes.sizeof(s)
        self._call("stats", ctypes.byref(s))
        return s.asdict()

    def diagnostics(self, first=0, count=None):
        """<prefix>_diagnostics: one dict per member of [first, first + count) (default: all from `first`).  Synchronises."""
        where = self._prefix + "_diagnostics"
        if not hasattr(self._L, where):
            raise NbxError(NBX_ERR_STATE, where, "%s was built without %s" % (LIB_PATH, where))
        count = self.members - first if count is None else count
        d = (Diag * max(count, 1))()
        for k in range(max(count, 0)):
            d[k].struct_size = ctypes.sizeof(Diag)
        self._call("diagnostics", first, count, d)
        return [d[k].asdict() for k in range(max(count, 0))]

    def timescale(self, first=0, count=None):
        """<prefix>_timescale: one dict per member of [first, first + count) (default: all from `first`), each what
        Context.timescale() returns for a context of the member's size holding its state -- the same bits; one launch for all of
        them.  Synchronises."""
        _need(self._L, self._prefix + "_timescale")
        count = self.members - first if count is None else count
        t = (Timescale * max(count, 1))()
        for k in range(max(count, 0)):
            t[k].struct_size = ctypes.sizeof(Timescale)
        self._call("timescale", first, count, t)
        return [t[k].asdict() for k in range(max(count, 0))]

    def field(self, px, py, pz, first=0, count=None):
        """<prefix>_field: the acceleration and the potential of members [first, first + count) (default: all from `first`), each
        at its own m points -- px, py, pz of shape (count, m), row k the points of member first + k -- as {"acc_x", "acc_y",
        "acc_z", "phi"}, arrays (count, m); for each member the bits Context.field() returns for a context of the member's size
        holding its state and given the same points; one launch for all of them.  Synchronises."""
        _need(self._L, self._prefix + "_field")
        count = self.members - first if count is None else count
        p = [np.ascontiguousarray(a, dtype=self.dtype) for a in (px, py, pz)]
        if p[0].ndim != 2 or p[0].shape[0] != max(count, 0) or any(a.shape != p[0].shape for a in p):
            raise NbxError(NBX_ERR_ARG, "array", "expected three arrays of shape (%d, m), got %r" % (max(count, 0), [a.shape for a in p]))
        m = p[0].shape[1]
        out = {k: np.zeros((max(count, 0), m), dtype=self.dtype) for k in FIELD_KEYS}
        self._call("field", first, count, m, *[_ptr(a) for a in p], *[_ptr(out[k]) for k in FIELD_KEYS])
        return out

    def tidal(self, px, py, pz, first=0, count=None):
        """<prefix>_tidal: the tidal tensor of members [first, first + count) (default: all from `first`), each at its own m
        points -- px, py, pz of shape (count, m), row k the points of member first + k -- as the six TIDAL_KEYS arrays
        (count, m); for each member the bits Context.tidal() returns for a context of the member's size holding its state and
        given the same points; one launch for all of them.  Synchronises."""
        _need(self._L, self._prefix + "_tidal")
        count = self.members - first if count is None else count
        p = [np.ascontiguousarray(a, dtype=self.dtype) for a in (px, py, pz)]
        if p[0].ndim != 2 or p[0].shape[0] != max(count, 0) or any(a.shape != p[0].shape for a in p):
            raise NbxError(NBX_ERR_ARG, "array", "expected three arrays of shape (%d, m), got %r" % (max(count, 0), [a.shape for a in p]))
        m = p[0].shape[1]
        out, t = _tidal_arrays((max(count, 0), m), self.dtype)
        self._call("tidal", first, count, m, *[_ptr(a) for a in p], t)
        return out

    def _tracers_call(self, name, *args):
        _need(self._L, "%s_tracers_%s" % (self._prefix, name))
        self._call("tracers_" + name, *args)

    def _tracers_range(self, first, count, default=False):
        if count is None:
            if not default:
                raise NbxError(NBX_ERR_ARG, "array", "expected arrays of shape (count, m)")
            count = self.members - first
        return (first, count), (max(count, 0),)

    def _accel(self, first, count, arrs):
        """<prefix>_accel into three host arrays (None skips one).  Synchronises."""
        where = self._prefix + "_accel"
        if not hasattr(self._L, where):
            raise NbxError(NBX_ERR_STATE, where, "%s was built without %s" % (LIB_PATH, where))
        self._call("accel", first, count, *[_ptr(a) for a in arrs])


class Ensemble(_Batch):
    """One nbx_ensemble (include/nbx_ensemble.h): `members` independent systems of n bodies, one launch per time step for all
    of them.  Keyword options are the nbx_opts fields an ensemble honours (device, bodies_per_lane, inner_loop)."""
    _prefix, _stats, _what = "nbx_ensemble", EnsembleStats, "the ensemble entry points"

    def __init__(self, n, members, precision=32, **opts):
        self.n, self.members, self.precision = int(n), int(members), int(precision)
        self._create(opts, self.n, self.precision, self.members)

    def upload(self, states, first=0):
        """Members first, first + 1, ...: a list of state dicts (what initial_conditions returns), or one dict of (count, n) arrays."""
        if isinstance(states, dict):
            arrs = [np.ascontiguousarray(states[f], dtype=self.dtype) for f in FIELDS]
        else:
            arrs = [np.ascontiguousarray(np.stack([np.asarray(s[f]) for s in states]), dtype=self.dtype) for f in FIELDS]
        for a in arrs:
            if a.ndim != 2 or a.shape != (arrs[0].shape[0], self.n):
                raise NbxError(NBX_ERR_ARG, "array", "expected shape (count, %d), got %r" % (self.n, a.shape))
        self._call("upload", first, arrs[0].shape[0], *[_ptr(a) for a in arrs])
        _remember_mass(self, first, arrs[6])

    def download(self, first=0, count=None):
        count = self.members - first if count is None else count
        out = {f: np.zeros((max(count, 0), self.n), dtype=self.dtype) for f in FIELDS[:6]}
        self._call("download", first, count, *[_ptr(out[f]) for f in FIELDS[:6]])
        return out

    def accel(self, first=0, count=None):
        """nbx_ensemble_accel: [ax, ay, az], each (count, n), of members [first, first + count) (default: all from `first`) at the
        current positions -- for each member the bits Context.accel() returns for a jlane context of n bodies holding its state;
        one launch for all of them.  Synchronises."""
        count = self.members - first if count is None else count
        a = [np.zeros((max(count, 0), self.n), dtype=self.dtype) for _ in range(3)]
        self._accel(first, count, a)
        return a

    def neighbours(self, radius=None, first=0, count=None):
        """nbx_ensemble_neighbours: {"index", "r2", "within"}, arrays (count, n), of members [first, first + count) (default: all
        from `first`) -- for each member the bits Context.neighbours() returns for a context of n bodies holding its state; one
        launch for all of them.  within is None when radius is None.  Synchronises."""
        _need(self._L, "nbx_ensemble_neighbours")
        count = self.members - first if count is None else count
        out = _neighbour_arrays((max(count, 0), self.n), self.dtype, radius)
        self._call("neighbours", first, count, 0.0 if radius is None else radius, *[_ptr(out[k]) for k in NEIGHBOUR_KEYS])
        return out

    def knn(self, k, first=0, count=None):
        """nbx_ensemble_knn: {"index", "r2"}, arrays (count, n, k), of members [first, first + count) (default: all from `first`)
        -- for each member the bits Context.knn(k) returns for a context of n bodies holding its state; one launch for all of
        them.  Synchronises."""
        _need(self._L, "nbx_ensemble_knn")
        count = self.members - first if count is None else count
        rows = max(count, 0) * self.n
        flat = _knn_arrays(rows, k, self.dtype)
        self._call("knn", first, count, k, *[_ptr(flat[key]) for key in KNN_KEYS])
        return {key: flat[key][:rows * k].reshape(max(count, 0), self.n, k) for key in KNN_KEYS}

    def tidal_bodies(self, first=0, count=None):
        """nbx_ensemble_tidal_bodies: the six TIDAL_KEYS arrays (count, n) of members [first, first + count) (default: all from
        `first`) -- for each member the bits Context.tidal_bodies() returns for a context of n bodies holding its state; one
        launch for all of them.  Synchronises."""
        _need(self._L, "nbx_ensemble_tidal_bodies")
        count = self.members - first if count is None else count
        out, t = _tidal_arrays((max(count, 0), self.n), self.dtype)
        self._call("tidal_bodies", first, count, t)
        return out

    def clumps(self, label, first=0, count=None):
        """nbx_ensemble_clumps: under the int32 labels `label` (count, n), member-local, the ten CLUMPS_KEYS arrays (count, n) of
        members [first, first + count) (default: all from `first`) -- for each member the bits Context.clumps() returns for a
        context of n bodies holding its state and labels; one launch for all of them.  Synchronises."""
        _need(self._L, "nbx_ensemble_clumps")
        count = self.members - first if count is None else count
        lab = _clumps_label(label, (max(count, 0), self.n))
        out, a = _clumps_arrays((max(count, 0), self.n), self.dtype)
        self._call("clumps", first, count, _ptr(lab), ctypes.byref(a))
        return out

    def jerk(self, first=0, count=None):
        """nbx_ensemble_jerk: the six JERK_KEYS arrays (count, n) of members [first, first + count) (default: all from `first`)
        -- for each member the bits Context.jerk() returns for a context of n bodies holding its state; one launch for all of
        them.  Synchronises."""
        _need(self._L, "nbx_ensemble_jerk")
        count = self.members - first if count is None else count
        out, a = _jerk_arrays((max(count, 0), self.n), self.dtype)
        self._call("jerk", first, count, ctypes.byref(a))
        return out

    def binaries(self, bound=True, first=0, count=None):
        """nbx_ensemble_binaries: {"partner", "energy", "bound"}, arrays (count, n), of members [first, first + count) (default:
        all from `first`) -- for each member the bits Context.binaries() returns for a context of n bodies holding its state; one
        launch for all of them.  bound is None when bound=False.  Synchronises."""
        _need(self._L, "nbx_ensemble_binaries")
        count = self.members - first if count is None else count
        out = _binaries_arrays((max(count, 0), self.n), self.dtype, bound)
        self._call("binaries", first, count, *[_ptr(out[k]) for k in BINARIES_KEYS])
        return out

    def fof(self, radius, first=0, count=None):
        """nbx_ensemble_fof: {"label", "size"}, int32 arrays (count, n), {"groups", "largest"}, int32 arrays (count,), and
        "passes", the call's, of members [first, first + count) (default: all from `first`) -- for each member the labels and
        sizes Context.fof() returns for a context of n bodies holding its state; every pass is one launch for all of them.
        Synchronises once per pass."""
        _need(self._L, "nbx_ensemble_fof")
        count = self.members - first if count is None else count
        S = max(count, 0)
        label, size, info, passes = _fof_arrays(S * self.n, S)
        self._call("fof", first, count, radius, _ptr(label), _ptr(size), _ptr(info), _ptr(passes))
        return {"label": label[:S * self.n].reshape(S, self.n), "size": size[:S * self.n].reshape(S, self.n), "groups": info[:S, 0].copy(),
                "largest": info[:S, 1].copy(), "passes": int(passes[0])}

    def nlist(self, radius, capacity=None, first=0, count=None):
        """nbx_ensemble_nlist: what Context.nlist() returns, for members [first, first + count) (default: all from `first`) in one
        result: offsets (count * n + 1,) run across the members, body i of member first + k is at k * n + i, the indices are
        member-local -- for each member the bits Context.nlist() returns for a context of n bodies holding its state.
        nbx.nlist_pairs(result, n) splits it by member."""
        _need(self._L, "nbx_ensemble_nlist")
        count = self.members - first if count is None else count
        return _nlist(lambda *a: self._call("nlist", first, count, *a), max(count, 0) * self.n, self.dtype, radius, capacity)

    def paircount(self, radii, first=0, count=None):
        """nbx_ensemble_paircount: a np.uint64 array (count, len(radii)) of members [first, first + count) (default: all from
        `first`) -- for each member the bits Context.paircount() returns for a context of n bodies holding its state; one launch
        per 16 radii for all of them.  Synchronises."""
        return _batch_paircount(self, radii, first, count)

    def diagnostics(self, first=0, count=None):
        """nbx_ensemble_diagnostics: one dict per member of [first, first + count) (default: all from `first`), each what
        Context.diagnostics() returns for a context of n bodies holding that member's state -- the same bits; one launch for
        all of them.  Synchronises."""
        return super().diagnostics(first, count)


class Ragged(_Batch):
    """One nbx_ragged (include/nbx_ragged.h): independent systems of different size, member k of sizes[k] bodies, one launch per
    time step for all of them.  Keyword options are the nbx_opts fields it honours (device, bodies_per_lane, inner_loop)."""
    _prefix, _stats, _what = "nbx_ragged", RaggedStats, "the ragged-ensemble entry points"

    def __init__(self, sizes, precision=32, **opts):
        self.sizes = [int(n) for n in sizes]
        self.members, self.precision = len(self.sizes), int(precision)
        self._create(opts, self.members, (ctypes.c_int32 * max(self.members, 1))(*self.sizes), self.precision)

    def _range(self, first, count):
        """The sizes of members [first, first + count), or [] where the range leaves [0, members) (the library names the error)."""
        return self.sizes[first:first + count] if 0 <= first and 0 <= count and first + count <= self.members else []

    def upload(self, states, first=0):
        """Members first, first + 1, ...: a list of state dicts (what initial_conditions returns), member first + k of sizes[first + k] bodies."""
        states = list(states)
        sizes = self._range(first, len(states))
        for k, n in enumerate(sizes):
            for f in FIELDS:
                if np.shape(states[k][f]) != (n,):
                    raise NbxError(NBX_ERR_ARG, "array", "member %d: expected shape (%d,), got %r" % (first + k, n, np.shape(states[k][f])))
        arrs = [np.ascontiguousarray(np.concatenate([np.asarray(s[f], dtype=self.dtype) for s in states]) if states
                                     else np.zeros(0, dtype=self.dtype)) for f in FIELDS]
        self._call("upload", first, len(states), *[_ptr(a) for a in arrs])
        _remember_mass(self, first, [s["mass"] for s in states])

    def download(self, first=0, count=None):
        """Members [first, first + count) (default: all from `first`): a list of dicts of six arrays, one per member."""
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        flat = {f: np.zeros(max(sum(sizes), 1), dtype=self.dtype) for f in FIELDS[:6]}
        self._call("download", first, count, *[_ptr(flat[f]) for f in FIELDS[:6]])
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [{f: flat[f][at[k]:at[k + 1]].copy() for f in FIELDS[:6]} for k in range(len(sizes))]

    def accel(self, first=0, count=None):
        """nbx_ragged_accel: one [ax, ay, az] per member of [first, first + count) (default: all from `first`) at the current
        positions -- the bits Context.accel() returns for a jlane context of sizes[k] bodies holding that member's state; one
        launch for all of them.  Synchronises."""
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        flat = [np.zeros(max(sum(sizes), 1), dtype=self.dtype) for _ in range(3)]  # >= 1: _ptr wants an address, also for an empty range
        self._accel(first, count, flat)
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [[a[at[k]:at[k + 1]].copy() for a in flat] for k in range(len(sizes))]

    def neighbours(self, radius=None, first=0, count=None):
        """nbx_ragged_neighbours: one {"index", "r2", "within"} per member of [first, first + count) (default: all from `first`),
        arrays of sizes[k] -- the bits Context.neighbours() returns for a context of sizes[k] bodies holding that member's state;
        one launch for all of them.  within is None when radius is None.  Synchronises."""
        _need(self._L, "nbx_ragged_neighbours")
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        flat = _neighbour_arrays((max(sum(sizes), 1),), self.dtype, radius)  # >= 1: _ptr wants an address, also for an empty range
        self._call("neighbours", first, count, 0.0 if radius is None else radius, *[_ptr(flat[k]) for k in NEIGHBOUR_KEYS])
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [{k: None if flat[k] is None else flat[k][at[m]:at[m + 1]].copy() for k in NEIGHBOUR_KEYS} for m in range(len(sizes))]

    def knn(self, k, first=0, count=None):
        """nbx_ragged_knn: one {"index", "r2"} per member of [first, first + count) (default: all from `first`), arrays
        (sizes[m], k) -- the bits Context.knn(k) returns for a context of sizes[m] bodies holding that member's state; one launch
        for all of them.  Synchronises."""
        _need(self._L, "nbx_ragged_knn")
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        flat = _knn_arrays(sum(sizes), k, self.dtype)
        self._call("knn", first, count, k, *[_ptr(flat[key]) for key in KNN_KEYS])
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int) * max(int(k), 0)
        return [{key: flat[key][at[m]:at[m + 1]].reshape(sizes[m], k).copy() for key in KNN_KEYS} for m in range(len(sizes))]

    def tidal_bodies(self, first=0, count=None):
        """nbx_ragged_tidal_bodies: the six TIDAL_KEYS arrays of members [first, first + count) (default: all from `first`), ONE
        array per key with the members end to end (member first + k at sum(sizes[first:first + k])) -- for each member the bits
        Context.tidal_bodies() returns for a context of its size holding its state; one launch for all of them.  Synchronises."""
        _need(self._L, "nbx_ragged_tidal_bodies")
        count = self.members - first if count is None else count
        total = sum(self._range(first, count))
        out, t = _tidal_arrays(max(total, 1), self.dtype)  # >= 1: an address is wanted, also for an empty range
        self._call("tidal_bodies", first, count, t)
        return {k: out[k][:total] for k in TIDAL_KEYS}

    def clumps(self, label, first=0, count=None):
        """nbx_ragged_clumps: under `label`, a list of one int32 array of sizes[k] per member of [first, first + count) (default:
        all from `first`), member-local, one dict of the ten CLUMPS_KEYS arrays of sizes[k] per member -- the bits
        Context.clumps() returns for a context of sizes[k] bodies holding that member's state and labels; one launch for all of
        them.  Synchronises."""
        _need(self._L, "nbx_ragged_clumps")
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        label = [np.asarray(l) for l in label]
        if sizes and [l.shape for l in label] != [(n,) for n in sizes]:
            raise NbxError(NBX_ERR_ARG, "label", "expected one array of sizes[k] labels per member of the range")
        total = sum(sizes)
        lab = _clumps_label(np.concatenate(label) if sizes else np.zeros(0, dtype=np.int32), (total,))
        flat, a = _clumps_arrays((max(total, 1),), self.dtype)  # >= 1: an address is wanted, also for an empty range
        self._call("clumps", first, count, _ptr(lab), ctypes.byref(a))
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [{k: flat[k][at[m]:at[m + 1]].copy() for k in CLUMPS_KEYS} for m in range(len(sizes))]

    def jerk(self, first=0, count=None):
        """nbx_ragged_jerk: one dict of the six JERK_KEYS arrays of sizes[k] per member of [first, first + count) (default: all
        from `first`) -- the bits Context.jerk() returns for a context of sizes[k] bodies holding that member's state; one launch
        for all of them.  Synchronises."""
        _need(self._L, "nbx_ragged_jerk")
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        flat, a = _jerk_arrays((max(sum(sizes), 1),), self.dtype)  # >= 1: an address is wanted, also for an empty range
        self._call("jerk", first, count, ctypes.byref(a))
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [{k: flat[k][at[m]:at[m + 1]].copy() for k in JERK_KEYS} for m in range(len(sizes))]

    def binaries(self, bound=True, first=0, count=None):
        """nbx_ragged_binaries: one {"partner", "energy", "bound"} per member of [first, first + count) (default: all from
        `first`), arrays of sizes[k] -- the bits Context.binaries() returns for a context of sizes[k] bodies holding that member's
        state, partner member-local; one launch for all of them.  bound is None when bound=False.  Synchronises."""
        _need(self._L, "nbx_ragged_binaries")
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        flat = _binaries_arrays((max(sum(sizes), 1),), self.dtype, bound)  # >= 1: _ptr wants an address, also for an empty range
        self._call("binaries", first, count, *[_ptr(flat[k]) for k in BINARIES_KEYS])
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [{k: None if flat[k] is None else flat[k][at[m]:at[m + 1]].copy() for k in BINARIES_KEYS} for m in range(len(sizes))]

    def fof(self, radius, first=0, count=None):
        """nbx_ragged_fof: one {"label", "size", "groups", "largest", "passes"} per member of [first, first + count) (default:
        all from `first`), label and size int32 arrays of sizes[m] -- what Context.fof() returns for a context of sizes[m]
        bodies holding that member's state, but for "passes", which is the call's: the largest of the members' own; every pass
        is one launch for all of them.  Synchronises once per pass."""
        _need(self._L, "nbx_ragged_fof")
        count = self.members - first if count is None else count
        sizes = self._range(first, count)
        label, size, info, passes = _fof_arrays(sum(sizes), len(sizes))
        self._call("fof", first, count, radius, _ptr(label), _ptr(size), _ptr(info), _ptr(passes))
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        return [{"label": label[at[m]:at[m + 1]].copy(), "size": size[at[m]:at[m + 1]].copy(), "groups": int(info[m, 0]),
                 "largest": int(info[m, 1]), "passes": int(passes[0])} for m in range(len(sizes))]

    def nlist(self, radius, capacity=None, first=0, count=None):
        """nbx_ragged_nlist: what Context.nlist() returns, for members [first, first + count) (default: all from `first`) in one
        result: the members' bodies end to end, offsets run across them, the indices are member-local -- for each member the
        bits Context.nlist() returns for a context of sizes[k] bodies holding its state.  nbx.nlist_pairs(result, sizes of the
        range) splits it by member."""
        _need(self._L, "nbx_ragged_nlist")
        count = self.members - first if count is None else count
        return _nlist(lambda *a: self._call("nlist", first, count, *a), sum(self._range(first, count)), self.dtype, radius, capacity)

    def paircount(self, radii, first=0, count=None):
        """nbx_ragged_paircount: a np.uint64 array (count, len(radii)) of members [first, first + count) (default: all from
        `first`) -- for each member the bits Context.paircount() returns for a context of sizes[k] bodies holding its state; one
        launch per 16 radii for all of them.  Synchronises."""
        return _batch_paircount(self, radii, first, count)

    def diagnostics(self, first=0, count=None):
        """nbx_ragged_diagnostics: one dict per member of [first, first + count) (default: all from `first`), each what
        Context.diagnostics() returns for a context of sizes[k] bodies holding that member's state -- the same bits; one launch
        for all of them.  Synchronises."""
        return super().diagnostics(first, count)


class Group(_Handle, _Leapfrog):
    """One nbx_group: n_ranks contexts driven by this process (multi-GPU; logical ranks when devices repeat)."""
    _destroy = "nbx_group_destroy"

    def __init__(self, n, precision=32, n_ranks=1, devices=None, rank=None, unique_id=None, device=-1, weights=None, weighted=False, **opts):
        """Single process: n_ranks contexts on `devices`.  One process per GPU: pass rank= and unique_id= (the 128 bytes
        of unique_id() made on rank 0 and shipped to every rank); n_ranks is then the world size and every call on the
        group is collective (nbx_group_create_rank).  weights= (or weighted=True for equal weights): unequal shares in whole
        256-record tiles (nbx_group_create_weighted), which retune() can move."""
        self._new_handle()
        self.n, self.precision, self.dtype = int(n), int(precision), _dtype(precision)
        o = _opts(opts)  # the library sets the device of every rank itself
        if rank is not None:
            buf = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
            _check(self._L.nbx_group_create_rank(ctypes.byref(self._h), self.n, self.precision, n_ranks, rank, buf, device, ctypes.byref(o)),
                   "nbx_group_create_rank")
            return
        dev = None if devices is None else (ctypes.c_int32 * len(devices))(*devices)
        if weights is not None or weighted:
            w = None if weights is None else (ctypes.c_double * len(weights))(*weights)
            _check(self._L.nbx_group_create_weighted(ctypes.byref(self._h), self.n, self.precision, n_ranks, dev, w, ctypes.byref(o)),
                   "nbx_group_create_weighted")
            return
        _check(self._L.nbx_group_create(ctypes.byref(self._h), self.n, self.precision, n_ranks, dev, ctypes.byref(o)),
               "nbx_group_create")

    def __del__(self):  # never with the Python object: the destroy of a rank group is collective, and only close() starts one
        pass

    def upload(self, state):
        arrs = [np.ascontiguousarray(state[f], dtype=self.dtype) for f in FIELDS]
        _check(self._L.nbx_group_upload(self._h, *[_ptr(a) for a in arrs]), "nbx_group_upload")

    def step(self, nsteps, dt=DT, kenergy=True):
        ke = ctypes.c_double(0.0)
        _check(self._L.nbx_group_step(self._h, dt, nsteps, ctypes.byref(ke) if kenergy else None), "nbx_group_step")
        return ke.value if kenergy else None

    def kick(self, h, kenergy=False):
        """nbx_group_kick: every rank kicks its owned slice; with kenergy the ranks' sums are added as step() adds them
        (collective for rank groups)."""
        _need(self._L, "nbx_group_kick")
        ke = ctypes.c_double(0.0)
        _check(self._L.nbx_group_kick(self._h, h, ctypes.byref(ke) if kenergy else None), "nbx_group_kick")
        return ke.value if kenergy else None

    def diagnostics(self):
        """nbx_group_diagnostics: system totals summed over the ranks in rank order (collective for rank groups), plus
        etotal = kenergy + potential."""
        d = Diag()
        d.struct_size = ctypes.sizeof(Diag)
        _check(self._L.nbx_group_diagnostics(self._h, ctypes.byref(d)), "nbx_group_diagnostics")
        return d.asdict()

    def download(self):
        out = {f: np.zeros(self.n, dtype=self.dtype) for f in FIELDS[:6]}
        _check(self._L.nbx_group_download(self._h, *[_ptr(out[f]) for f in FIELDS[:6]]), "nbx_group_download")
        return out

    def shares(self, timings=True):
        """nbx_group_shares: (i_begin list, i_count list, mean force-kernel ms per rank since the last retune)."""
        P = self.info(0)[0]
        b, c, ms = (ctypes.c_int32 * P)(), (ctypes.c_int32 * P)(), (ctypes.c_double * P)()
        _check(self._L.nbx_group_shares(self._h, b, c, ms if timings else None), "nbx_group_shares")
        return list(b), list(c), list(ms)

    def retune(self, force_ms=None):
        """nbx_group_retune: new shares from the measured (or the given) per-rank force-kernel times; True if they moved."""
        ch = ctypes.c_int32(0)
        ms = None if force_ms is None else (ctypes.c_double * len(force_ms))(*force_ms)
        _check(self._L.nbx_group_retune(self._h, ms, ctypes.byref(ch)), "nbx_group_retune")
        return bool(ch.value)

    def info(self, rank=0):
        P, rccl, st = ctypes.c_int32(), ctypes.c_int32(), Stats()
        _check(self._L.nbx_group_info(self._h, ctypes.byref(P), ctypes.byref(rccl), rank, ctypes.byref(st)), "nbx_group_info")
        return P.value, bool(rccl.value), st.asdict()


UNIQUE_ID_BYTES = 128


def unique_id():
    """nbx_comm_unique_id: the rendezvous token rank 0 creates for a one-process-per-GPU group."""
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    _check(load().nbx_comm_unique_id(buf), "nbx_comm_unique_id")
    return buf.raw


EXIT_COLLECTIVE_TIMEOUT = 75


def collective_timeout(seconds):
    """nbx_collective_timeout: the watchdog's bound on blocking group collectives (<= 0: off)."""
    _check(load().nbx_collective_timeout(float(seconds)), "nbx_collective_timeout")


def partition(n, n_ranks, rank):
    """nbx_partition: (ranks_used, block, i_begin, i_count, n_alloc) of the library's block partition."""
    out = [ctypes.c_int32() for _ in range(5)]
    _check(load().nbx_partition(n, n_ranks, rank, *[ctypes.byref(o) for o in out]), "nbx_partition")
    return tuple(o.value for o in out)


def partition_weighted(n, n_ranks, weights, rank):
    """nbx_partition_weighted: (ranks_used, i_begin, i_count, n_alloc); weights None = equal."""
    out = [ctypes.c_int32() for _ in range(4)]
    w = None if weights is None else (ctypes.c_double * len(weights))(*weights)
    _check(load().nbx_partition_weighted(n, n_ranks, w, rank, *[ctypes.byref(o) for o in out]), "nbx_partition_weighted")
    return tuple(o.value for o in out)


def tune_weights(i_count, force_ms):
    """nbx_tune_weights: the tuner's arithmetic (each rank's measured bodies per millisecond, normalised)."""
    P = len(i_count)
    out = (ctypes.c_double * P)()
    _check(load().nbx_tune_weights(P, (ctypes.c_int32 * P)(*i_count), (ctypes.c_double * P)(*force_ms), out), "nbx_tune_weights")
    return list(out)


def read_snapshot(path):
    """Read an NBXSNAP1 file written by nbody.x (NBODY_SNAPSHOT=...): returns (state dict, steps_done)."""
    import struct
    with open(path, "rb") as f:
        magic, n, prec, steps = struct.unpack("<8siiq", f.read(24))
        if magic != b"NBXSNAP1":
            raise ValueError("%s is not an NBXSNAP1 snapshot" % path)
        dt = _dtype(prec)
        state = {k: np.frombuffer(f.read(n * dt().itemsize), dtype=dt).copy() for k in FIELDS}
    return state, steps
