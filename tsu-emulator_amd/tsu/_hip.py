"""ctypes binding of libtsu_hip.so (include/tsu_hip.h) -- the only door to the GPU.

There is deliberately no CPU fallback in this package: if the HIP library is missing or no GPU is
present, every operation that needs it raises :class:`HipUnavailableError`.
"""
import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TSU_HIP_LIB") or os.path.join(_HERE, "_lib", "libtsu_hip.so")  # (TSU_HIP_LIB: development builds)

TSU_OK = 0
TSU_E_INVALID, TSU_E_NOMEM, TSU_E_HIP, TSU_E_RCCL, TSU_E_UNSUPPORTED = -1, -2, -3, -4, -5
MODE_PHYSICAL, MODE_COMPAT = 0, 1
DTYPE_F64, DTYPE_F32 = 0, 1
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED, KERNEL_SMALL = 0, 1, 2, 3
PART_ALL, PART_INTERIOR, PART_BOUNDARY = 0, 1, 2


class HipUnavailableError(RuntimeError):
    """libtsu_hip.so is not built / not loadable, or there is no HIP device."""


class HipError(RuntimeError):
    """A call into libtsu_hip.so failed (TSU_E_HIP / TSU_E_NOMEM / TSU_E_RCCL)."""


class UnsupportedError(HipError):
    """TSU_E_UNSUPPORTED: valid request the HIP build has no kernel for."""


_u8p, _i8p = C.POINTER(C.c_uint8), C.POINTER(C.c_int8)
_u32p, _u64p, _i64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_f32p, _f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes): mirrors include/tsu_hip.h one to one (tests check every symbol exists)
SIGNATURES = {
    "tsu_version": (C.c_int, []),
    "tsu_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "tsu_shutdown": (C.c_int, [_vp]),
    "tsu_last_error": (C.c_char_p, [_vp]),
    "tsu_set_stream": (C.c_int, [_vp, _vp]),
    "tsu_synchronize": (C.c_int, [_vp]),
    "tsu_device_info": (C.c_int, [_vp, C.c_char_p, C.c_int, C.POINTER(C.c_int), _u64p]),
    "tsu_timer_begin": (C.c_int, [_vp]),
    "tsu_timer_end": (C.c_int, [_vp, _f32p]),
    "tsu_philox4x32_10": (C.c_int, [_vp, C.c_int, _u32p, _u32p, _u32p]),
    "tsu_ising2d_thresholds": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int, _u64p]),
    "tsu_ising2d_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_ising2d_create_slab": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int,
                                          C.POINTER(_vp)]),
    "tsu_ising2d_destroy": (C.c_int, [_vp]),
    "tsu_ising2d_set_spins": (C.c_int, [_vp, _i8p, C.c_int, C.c_int]),
    "tsu_ising2d_get_spins": (C.c_int, [_vp, _i8p, C.c_int, C.c_int]),
    "tsu_ising2d_randomize": (C.c_int, [_vp, C.c_uint64, C.c_uint32]),
    "tsu_ising2d_fill": (C.c_int, [_vp, C.c_int8]),
    "tsu_ising2d_set_thresholds": (C.c_int, [_vp, _u64p]),
    "tsu_ising2d_set_model": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_int]),
    "tsu_ising2d_set_kernel": (C.c_int, [_vp, C.c_int, C.c_int]),
    "tsu_ising2d_sweep": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_ising2d_sweep_part": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]),
    "tsu_ising2d_observables": (C.c_int, [_vp, _i64p, _i64p]),
    "tsu_ising2d_sample": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, _i8p]),
    "tsu_ising2d_sweep_batch": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]),
    "tsu_ising2d_observables_batch": (C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsu_ising2d_row_ptr": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "tsu_ising2d_set_timing": (C.c_int, [_vp, C.c_int]),
    "tsu_ising2d_last_sweep_ms": (C.c_int, [_vp, _f32p]),
    "tsu_ising2d_launch_count": (C.c_int, [_vp, _u64p]),
    "tsu_ising2d_strip_numbering": (C.c_int, [_vp, _u32p, _u64p]),
    "tsu_ising2d_cluster_threshold": (C.c_int, [C.c_double, C.c_double, _u64p]),
    "tsu_ising2d_cluster_sweep": (C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_ising2d_cluster_sweep_batch": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tsu_ising2d_cluster_launch_count": (C.c_int, [_vp, _u64p]),
    "tsu_ising2d_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p]),
    "tsu_ising2d_clear_disorder": (C.c_int, [_vp]),
    "tsu_ising2d_disorder_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_ising2d_disorder_energy": (C.c_int, [_vp, _f64p]),
    "tsu_ising2d_overlap": (C.c_int, [_vp, _vp, _i64p]),
    "tsu_ising2d_disorder_launch_count": (C.c_int, [_vp, _u64p]),
    "tsu_pt2d_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_pt2d_destroy": (C.c_int, [_vp]),
    "tsu_pt2d_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p]),
    "tsu_pt2d_set_temperatures": (C.c_int, [_vp, _f64p]),
    "tsu_pt2d_init": (C.c_int, [_vp, C.c_uint64, C.c_int]),
    "tsu_pt2d_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tsu_pt2d_history": (C.c_int, [_vp, _f64p, _i64p, _i64p, _i32p]),
    "tsu_pt2d_stats": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i32p, _u64p, _u64p]),
    "tsu_pt2d_energies": (C.c_int, [_vp, _f64p, _i64p]),
    "tsu_pt2d_get_spins": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_pt2d_set_spins": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_pt2d_launch_count": (C.c_int, [_vp, _u64p]),
    "tsu_pt2d_set_cluster_moves": (C.c_int, [_vp, C.c_int, C.c_double]),
    "tsu_pt2d_cluster_move": (C.c_int, [_vp]),
    "tsu_pt2d_cluster_stats": (C.c_int, [_vp, _i64p, _i64p, _i64p, _u64p, _u64p]),
    "tsu_ising3d_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_ising3d_destroy": (C.c_int, [_vp]),
    "tsu_ising3d_set_spins": (C.c_int, [_vp, _i8p]),
    "tsu_ising3d_get_spins": (C.c_int, [_vp, _i8p]),
    "tsu_ising3d_randomize": (C.c_int, [_vp, C.c_uint64, C.c_uint32]),
    "tsu_ising3d_fill": (C.c_int, [_vp, C.c_int8]),
    "tsu_ising3d_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p]),
    "tsu_ising3d_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_ising3d_energy": (C.c_int, [_vp, _f64p]),
    "tsu_ising3d_sum_spins": (C.c_int, [_vp, _i64p]),
    "tsu_ising3d_overlap": (C.c_int, [_vp, _vp, _i64p]),
    "tsu_ising3d_launch_count": (C.c_int, [_vp, _u64p]),
    "tsu_pt3d_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_pt3d_destroy": (C.c_int, [_vp]),
    "tsu_pt3d_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p]),
    "tsu_pt3d_set_temperatures": (C.c_int, [_vp, _f64p]),
    "tsu_pt3d_init": (C.c_int, [_vp, C.c_uint64, C.c_int]),
    "tsu_pt3d_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tsu_pt3d_history": (C.c_int, [_vp, _f64p, _i64p, _i64p, _i32p]),
    "tsu_pt3d_stats": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i32p, _u64p, _u64p]),
    "tsu_pt3d_energies": (C.c_int, [_vp, _f64p, _i64p]),
    "tsu_pt3d_get_spins": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_pt3d_set_spins": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_pt3d_launch_count": (C.c_int, [_vp, _u64p]),
    "tsu_comm_unique_id": (C.c_int, [_u8p]),
    "tsu_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, _u8p, C.POINTER(_vp)]),
    "tsu_comm_destroy": (C.c_int, [_vp]),
    "tsu_ising2d_halo_exchange": (C.c_int, [_vp, _vp]),
    "tsu_comm_wait": (C.c_int, [_vp, C.c_double, _u64p]),
    "tsu_comm_allreduce_i64": (C.c_int, [_vp, _i64p, C.c_int]),
    "tsu_dense_create": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _f64p, C.POINTER(_vp)]),
    "tsu_dense_destroy": (C.c_int, [_vp]),
    "tsu_dense_set_state": (C.c_int, [_vp, _i8p]),
    "tsu_dense_get_state": (C.c_int, [_vp, _i8p]),
    "tsu_dense_sweep": (C.c_int, [_vp, C.c_double, C.c_int, _i64p, C.c_uint64, C.c_uint32, C.c_uint32, _f64p]),
    "tsu_dense_sample": (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.c_int, _i64p, C.c_uint64, C.c_uint32, C.c_uint32, _f64p, _i8p]),
    "tsu_dense_anneal": (C.c_int, [_vp, _f64p, C.c_int, _i64p, C.c_uint64, C.c_uint32, C.c_uint32, _f64p, _i8p]),
    "tsu_dense_sweep_replicas": (C.c_int, [_vp, C.c_int, _f64p, C.c_int, _i8p, _u64p, _u32p, _u32p, _f64p]),
    "tsu_dense_energy": (C.c_int, [_vp, _f64p]),
    "tsu_dense_energies": (C.c_int, [_vp, _i8p, C.c_int, _f64p]),
    "tsu_dense_launch_counts": (C.c_int, [_vp, _u64p]),
    "tsu_sparse_create": (C.c_int, [_vp, C.c_int, _i64p, _i32p, _f64p, _f64p, C.c_int, _i32p, _i32p, C.POINTER(_vp)]),
    "tsu_sparse_destroy": (C.c_int, [_vp]),
    "tsu_sparse_set_state": (C.c_int, [_vp, _i8p]),
    "tsu_sparse_get_state": (C.c_int, [_vp, _i8p]),
    "tsu_sparse_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_sparse_sample": (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, _i8p]),
    "tsu_sparse_energy": (C.c_int, [_vp, _f64p, _i64p]),
    "tsu_sparse_classify": (C.c_int, [C.c_int, _i64p, _i32p, _f64p, _f64p, C.c_int, _i32p, _i32p, _i32p]),
    "tsu_sparse_class_plan": (C.c_int, [_vp, C.c_int, _i32p]),
    "tsu_langevin_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_langevin_destroy": (C.c_int, [_vp]),
    "tsu_langevin_set_state": (C.c_int, [_vp, _f32p]),
    "tsu_langevin_get_state": (C.c_int, [_vp, _f32p]),
    "tsu_langevin_set_energy": (C.c_int, [_vp, _f32p, _f32p]),
    "tsu_langevin_set_coupling": (C.c_int, [_vp, _f32p, _f32p]),
    "tsu_langevin_set_mixture": (C.c_int, [_vp, C.c_int, _f32p, _f32p, _f32p, C.c_float]),
    "tsu_langevin_restart": (C.c_int, [_vp, _f32p, C.c_float, C.c_uint64, C.c_uint32]),
    "tsu_langevin_step": (C.c_int, [_vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_uint32,
                                    C.c_uint32, _f32p]),
    "tsu_langevin_set_kernel": (C.c_int, [_vp, C.c_int]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_ising3d_cluster.h (the header tsu_hip.h includes) one to one
CLUSTER3D_SIGNATURES = {
    "tsu_ising3d_cluster_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_ising3d_cluster_sweep_batch": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tsu_ising3d_cluster_launch_count": (C.c_int, [_vp, _u64p]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_correlation.h (the header tsu_hip.h includes) one to one
CORRELATION_SIGNATURES = {
    "tsu_ising2d_profiles": (C.c_int, [_vp, _vp, _i64p, _i64p]),
    "tsu_ising3d_profiles": (C.c_int, [_vp, _vp, _i64p, _i64p, _i64p]),
    "tsu_pt2d_set_correlation": (C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p, _f64p]),
    "tsu_pt3d_set_correlation": (C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]),
    "tsu_pt2d_history_modes": (C.c_int, [_vp, _f64p]),
    "tsu_pt3d_history_modes": (C.c_int, [_vp, _f64p]),
    "tsu_pt2d_profiles": (C.c_int, [_vp, C.c_int, _i64p, _i64p]),
    "tsu_pt3d_profiles": (C.c_int, [_vp, C.c_int, _i64p, _i64p, _i64p]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_population.h (the header tsu_hip.h includes) one to one
POPULATION_SIGNATURES = {}
for _pre, _shape, _nj in (("tsu_pa2d_", [C.c_int, C.c_int, C.c_int], 2), ("tsu_pa3d_", [C.c_int, C.c_int, C.c_int, C.c_int], 3)):
    POPULATION_SIGNATURES.update({
        _pre + "create": (C.c_int, [_vp] + _shape + [C.c_int, C.POINTER(_vp)]),
        _pre + "destroy": (C.c_int, [_vp]),
        _pre + "set_disorder": (C.c_int, [_vp] + [_f32p] * (_nj + 1)),
        _pre + "set_schedule": (C.c_int, [_vp, _f64p, C.c_int]),
        _pre + "init": (C.c_int, [_vp, C.c_uint64, C.c_int]),
        _pre + "run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        _pre + "history": (C.c_int, [_vp, _f64p, _i64p, _u32p, _i32p, _u64p, _u64p, _f64p]),
        _pre + "energies": (C.c_int, [_vp, _f64p, _i64p]),
        _pre + "get_spins": (C.c_int, [_vp, C.c_int, _i8p]),
        _pre + "set_spins": (C.c_int, [_vp, C.c_int, _i8p]),
        _pre + "launch_count": (C.c_int, [_vp, _u64p]),
    })

# name -> (restype, argtypes): mirrors include/tsu_hip_overlap.h (the header tsu_hip.h includes) one to one
OVERLAP_SIGNATURES = {
    "tsu_ising2d_link_overlap": (C.c_int, [_vp, _vp, _i64p, _i64p]),
    "tsu_ising3d_link_overlap": (C.c_int, [_vp, _vp, _i64p, _i64p]),
    "tsu_pt2d_set_link_overlap": (C.c_int, [_vp, C.c_int]),
    "tsu_pt3d_set_link_overlap": (C.c_int, [_vp, C.c_int]),
    "tsu_pt2d_history_link": (C.c_int, [_vp, _i64p]),
    "tsu_pt3d_history_link": (C.c_int, [_vp, _i64p]),
    "tsu_pa2d_set_overlap": (C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p, _f64p]),
    "tsu_pa3d_set_overlap": (C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]),
    "tsu_pa2d_history_overlap": (C.c_int, [_vp, _i64p, _i64p, _f64p]),
    "tsu_pa3d_history_overlap": (C.c_int, [_vp, _i64p, _i64p, _f64p]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_ensemble.h (the header tsu_hip.h includes) one to one
ENSEMBLE_SIGNATURES = {}
for _pre, _shape, _nj in (("tsu_pte2d_", [C.c_int, C.c_int, C.c_int], 2), ("tsu_pte3d_", [C.c_int, C.c_int, C.c_int, C.c_int], 3)):
    ENSEMBLE_SIGNATURES.update({
        _pre + "create": (C.c_int, [_vp] + _shape + [C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
        _pre + "destroy": (C.c_int, [_vp]),
        _pre + "set_disorder": (C.c_int, [_vp] + [_f32p] * (_nj + 1)),
        _pre + "set_temperatures": (C.c_int, [_vp, _f64p]),
        _pre + "init": (C.c_int, [_vp, _u64p, C.c_int]),
        _pre + "run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        _pre + "history": (C.c_int, [_vp, _f64p, _i64p, _i64p, _i32p]),
        _pre + "stats": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i32p, _u64p, _u64p]),
        _pre + "energies": (C.c_int, [_vp, _f64p, _i64p]),
        _pre + "get_spins": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i8p]),
        _pre + "set_spins": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i8p]),
        _pre + "launch_count": (C.c_int, [_vp, _u64p]),
        _pre + "set_correlation": (C.c_int, [_vp, C.c_int] + [_f64p] * (2 * (_nj if _nj == 2 else 3))),
        _pre + "history_modes": (C.c_int, [_vp, _f64p]),
        _pre + "set_link_overlap": (C.c_int, [_vp, C.c_int]),
        _pre + "history_link": (C.c_int, [_vp, _i64p]),
        _pre + "profiles": (C.c_int, [_vp, C.c_int, C.c_int] + [_i64p] * _nj),
    })

# name -> (restype, argtypes): mirrors include/tsu_hip_sparse_batch.h (the header tsu_hip.h includes) one to one
SPARSE_BATCH_SIGNATURES = {
    "tsu_sparse_batch_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_sparse_batch_destroy": (C.c_int, [_vp]),
    "tsu_sparse_batch_set_temperatures": (C.c_int, [_vp, _f64p]),
    "tsu_sparse_batch_init": (C.c_int, [_vp, C.c_uint64, C.c_int]),
    "tsu_sparse_batch_set_state": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_sparse_batch_get_state": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_sparse_batch_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tsu_sparse_batch_history": (C.c_int, [_vp, _f64p, _i64p, _i32p]),
    "tsu_sparse_batch_stats": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i32p, _u64p]),
    "tsu_sparse_batch_energies": (C.c_int, [_vp, _f64p, _i64p]),
    "tsu_sparse_batch_track_best": (C.c_int, [_vp, C.c_int]),
    "tsu_sparse_batch_best": (C.c_int, [_vp, C.c_int, _f64p, _i8p, _i32p]),
    "tsu_sparse_batch_plan": (C.c_int, [_vp, _i32p]),
    "tsu_sparse_batch_launch_count": (C.c_int, [_vp, _u64p]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_probe.h (the header tsu_hip.h includes) one to one
PROBE_SIGNATURES = {
    "tsu_probe_screen": (C.c_int, [_vp, C.c_int64, _f32p, _f32p, _f32p, _f32p, _f32p]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_cluster_field.h (the header tsu_hip.h includes) one to one
CLUSTER_FIELD_SIGNATURES = {
    "tsu_ising3d_cluster_sweep_field": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_ising3d_cluster_sweep_field_batch": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_multispin.h (the header tsu_hip.h includes) one to one
MULTISPIN_SIGNATURES = {
    "tsu_msc_thresholds": (C.c_int, [C.c_double, _u64p]),
    "tsu_msc_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_msc_destroy": (C.c_int, [_vp]),
    "tsu_msc_route": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "tsu_msc_set_couplings": (C.c_int, [_vp, _u64p, _u64p, _u64p]),
    "tsu_msc_set_planes": (C.c_int, [_vp, _u64p]),
    "tsu_msc_get_planes": (C.c_int, [_vp, _u64p]),
    "tsu_msc_set_seeds": (C.c_int, [_vp, _u64p]),
    "tsu_msc_randomize": (C.c_int, [_vp]),
    "tsu_msc_fill": (C.c_int, [_vp, C.c_int8]),
    "tsu_msc_set_temperatures": (C.c_int, [_vp, _f64p]),
    "tsu_msc_sweep": (C.c_int, [_vp, C.c_int, C.c_uint32]),
    "tsu_msc_measure": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i64p]),
    "tsu_msc_launch_count": (C.c_int, [_vp, _u64p]),
}
MSC_ROUTE_AUTO, MSC_ROUTE_SMALL, MSC_ROUTE_HBM = 0, 1, 2

# name -> (restype, argtypes): mirrors include/tsu_hip_multispin_pt.h (the header tsu_hip.h includes) one to one
MULTISPIN_PT_SIGNATURES = {
    "tsu_msc_pt_enable": (C.c_int, [_vp, _f64p]),
    "tsu_msc_pt_set_swap_seeds": (C.c_int, [_vp, _u64p]),
    "tsu_msc_pt_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32]),
    "tsu_msc_pt_stats": (C.c_int, [_vp, _i64p, _i64p, _i32p, _i32p, _i64p]),
    "tsu_msc_pt_history": (C.c_int, [_vp, C.c_int, _i64p, _i64p, _i64p, _i64p]),
    "tsu_msc_pt_launch_count": (C.c_int, [_vp, _u64p]),
}
MSC_PT_MAX_TEMPS = 256

# name -> (restype, argtypes): mirrors include/tsu_hip_multispin_corr.h (the header tsu_hip.h includes) one to one
MULTISPIN_CORR_SIGNATURES = {
    "tsu_msc_profiles": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "tsu_msc_set_correlation": (C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]),
    "tsu_msc_modes": (C.c_int, [_vp, _f64p]),
    "tsu_msc_pt_history_modes": (C.c_int, [_vp, C.c_int, _f64p]),
}

# name -> (restype, argtypes): mirrors include/tsu_hip_multispin_quench.h (the header tsu_hip.h includes) one to one
MULTISPIN_QUENCH_SIGNATURES = {
    "tsu_msc_c4": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "tsu_msc_snapshot_slots": (C.c_int, [_vp, C.c_int]),
    "tsu_msc_snapshot": (C.c_int, [_vp, C.c_int]),
    "tsu_msc_snapshot_overlap": (C.c_int, [_vp, C.c_int, _i64p]),
    "tsu_msc_quench_run": (C.c_int, [_vp, C.c_int, _i32p, C.c_uint32, C.c_int, _i32p]),
    "tsu_msc_quench_history": (C.c_int, [_vp, C.c_int, _i64p, _i64p, _i64p, _i64p, _i64p, _i64p, _i64p, _i64p]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_cluster_measure.h (the header tsu_hip.h includes) one to one
CLUSTER_MEASURE_SIGNATURES = {
    "tsu_ising2d_cluster_measure": (C.c_int, [_vp, C.c_int]),
    "tsu_ising3d_cluster_measure": (C.c_int, [_vp, C.c_int]),
    "tsu_ising2d_cluster_record": (C.c_int, [_vp, _i64p, C.c_int, C.POINTER(C.c_int)]),
    "tsu_ising3d_cluster_record": (C.c_int, [_vp, _i64p, C.c_int, C.POINTER(C.c_int)]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_potts.h (the header tsu_hip.h includes) one to one
POTTS_SIGNATURES = {
    "tsu_potts2d_check_model": (C.c_int, [C.c_int, C.c_double, _f64p, C.c_double, _f64p]),
    "tsu_potts2d_cluster_threshold": (C.c_int, [C.c_double, C.c_double, _u64p]),
    "tsu_potts2d_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_potts2d_destroy": (C.c_int, [_vp]),
    "tsu_potts2d_set_model": (C.c_int, [_vp, C.c_double, _f64p]),
    "tsu_potts2d_set_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts2d_get_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts2d_fill": (C.c_int, [_vp, C.c_int]),
    "tsu_potts2d_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts2d_cluster_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts2d_route": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "tsu_potts2d_measure": (C.c_int, [_vp, _i64p]),
    "tsu_potts2d_run": (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts2d_record": (C.c_int, [_vp, _i64p, C.c_int, C.POINTER(C.c_int)]),
    "tsu_potts2d_launch_count": (C.c_int, [_vp, _u64p]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_potts3d.h (the header tsu_hip.h includes) one to one
POTTS3D_SIGNATURES = {
    "tsu_potts3d_check_model": (C.c_int, [C.c_int, C.c_double, _f64p, C.c_double, _f64p]),
    "tsu_potts3d_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_potts3d_destroy": (C.c_int, [_vp]),
    "tsu_potts3d_set_model": (C.c_int, [_vp, C.c_double, _f64p]),
    "tsu_potts3d_set_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts3d_get_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts3d_fill": (C.c_int, [_vp, C.c_int]),
    "tsu_potts3d_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts3d_cluster_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts3d_route": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "tsu_potts3d_measure": (C.c_int, [_vp, _i64p]),
    "tsu_potts3d_run": (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts3d_record": (C.c_int, [_vp, _i64p, C.c_int, C.POINTER(C.c_int)]),
    "tsu_potts3d_launch_count": (C.c_int, [_vp, _u64p]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_potts_muca.h (the header tsu_hip.h includes) one to one
POTTS_MUCA_SIGNATURES = {
    "tsu_potts_muca_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, _i32p, _i64p, C.POINTER(C.c_int)]),
    "tsu_potts_muca_thresholds": (C.c_int, [C.c_int64, C.c_int, _f64p, _u64p]),
    "tsu_potts_muca_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.POINTER(_vp)]),
    "tsu_potts_muca_destroy": (C.c_int, [_vp]),
    "tsu_potts_muca_set_weights": (C.c_int, [_vp, _f64p, C.c_int64]),
    "tsu_potts_muca_set_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts_muca_get_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts_muca_fill": (C.c_int, [_vp, C.c_int]),
    "tsu_potts_muca_set_tunnel_bounds": (C.c_int, [_vp, C.c_int64, C.c_int64]),
    "tsu_potts_muca_run": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts_muca_energies": (C.c_int, [_vp, _i32p]),
    "tsu_potts_muca_tunnels": (C.c_int, [_vp, _u32p]),
    "tsu_potts_muca_record": (C.c_int, [_vp, _u64p, _u64p, _u64p]),
    "tsu_potts_muca_clear_record": (C.c_int, [_vp]),
    "tsu_potts_muca_measure": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "tsu_potts_muca_route": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "tsu_potts_muca_launch_count": (C.c_int, [_vp, _u64p]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_potts_disorder.h (the header tsu_hip.h includes) one to one
POTTS_DISORDER_SIGNATURES = {
    "tsu_potts_dis_site_thresholds": (C.c_int, [C.c_int, _f64p, C.c_double, _u64p]),
    "tsu_potts_dis_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.POINTER(_vp)]),
    "tsu_potts_dis_destroy": (C.c_int, [_vp]),
    "tsu_potts_dis_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p]),
    "tsu_potts_dis_set_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts_dis_get_spins": (C.c_int, [_vp, _i8p]),
    "tsu_potts_dis_fill": (C.c_int, [_vp, C.c_int]),
    "tsu_potts_dis_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts_dis_cluster_sweep": (C.c_int, [_vp, C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts_dis_route": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "tsu_potts_dis_measure": (C.c_int, [_vp, _i64p, _f64p]),
    "tsu_potts_dis_run": (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "tsu_potts_dis_record": (C.c_int, [_vp, _i64p, C.c_int, C.POINTER(C.c_int)]),
    "tsu_potts_dis_launch_count": (C.c_int, [_vp, _u64p]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_potts_pt.h (the header tsu_hip.h includes) one to one
POTTS_PT_SIGNATURES = {
    "tsu_potts_pt_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(_vp)]),
    "tsu_potts_pt_destroy": (C.c_int, [_vp]),
    "tsu_potts_pt_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p]),
    "tsu_potts_pt_set_temperatures": (C.c_int, [_vp, _f64p]),
    "tsu_potts_pt_set_spins": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_potts_pt_get_spins": (C.c_int, [_vp, C.c_int, C.c_int, _i8p]),
    "tsu_potts_pt_init": (C.c_int, [_vp, C.c_uint64, C.c_int]),
    "tsu_potts_pt_advance": (C.c_int, [_vp, C.c_uint64]),
    "tsu_potts_pt_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tsu_potts_pt_history": (C.c_int, [_vp, _f64p, _i64p, _i64p, _i32p]),
    "tsu_potts_pt_overlap_tables": (C.c_int, [_vp, _i64p]),
    "tsu_potts_pt_stats": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i32p, _u64p, _u64p]),
    "tsu_potts_pt_energies": (C.c_int, [_vp, _f64p, _i64p]),
    "tsu_potts_pt_route": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "tsu_potts_pt_launch_count": (C.c_int, [_vp, _u64p]),
}
# name -> (restype, argtypes): mirrors include/tsu_hip_potts_pop.h (the header tsu_hip.h includes) one to one
POTTS_POP_SIGNATURES = {
    "tsu_potts_pop_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.POINTER(_vp)]),
    "tsu_potts_pop_destroy": (C.c_int, [_vp]),
    "tsu_potts_pop_set_disorder": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p]),
    "tsu_potts_pop_set_schedule": (C.c_int, [_vp, _f64p, C.c_int]),
    "tsu_potts_pop_init": (C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int]),
    "tsu_potts_pop_advance": (C.c_int, [_vp, C.c_uint64]),
    "tsu_potts_pop_run": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tsu_potts_pop_history": (C.c_int, [_vp, _f64p, _i64p, _i64p, _u32p, _i32p, _u64p, _u64p, _f64p]),
    "tsu_potts_pop_energies": (C.c_int, [_vp, _f64p, _i64p]),
    "tsu_potts_pop_get_spins": (C.c_int, [_vp, C.c_int, _i8p]),
    "tsu_potts_pop_set_spins": (C.c_int, [_vp, C.c_int, _i8p]),
    "tsu_potts_pop_get_padded": (C.c_int, [_vp, C.c_int, _i8p]),
    "tsu_potts_pop_route": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "tsu_potts_pop_plan": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tsu_potts_pop_launch_count": (C.c_int, [_vp, _u64p]),
}
POTTS_POP_ROUTES = ("k14_pop_pack", "k14_pop_small", "k14_pop_sweep")  # TSU_POTTS_POP_ROUTE_*
POTTS_POP_MAX_WALKERS = 65535  # kPopMaxWalkers
POTTS_POP_DRAW = -2            # tsu_potts_pop_init's initial: the device draw
POTTS_PT_ROUTES = ("k13_pt_small", "k13_pt_sweep")  # TSU_POTTS_PT_ROUTE_*
POTTS_PT_MAX_TEMPS = 256  # kPtMaxTemps
POTTS_DIS_RECORD_WORDS = 10  # TSU_POTTS_DIS_RECORD_WORDS
POTTS_DIS_ROUTES = ("k12_small", "k12_sweep", "k12_sw_small", "k12_sw_tiles")  # TSU_POTTS_DIS_ROUTE_*
POTTS_MUCA_ROUTES = ("k11_muca_lds", "k11_muca_global", "k11_muca_atomics")  # TSU_POTTS_MUCA_ROUTE_*
POTTS_MUCA_MAX_SITES = 65536       # TSU_POTTS_MUCA_MAX_SITES
POTTS_MUCA_MAX_WALKERS = 1 << 20   # TSU_POTTS_MUCA_MAX_WALKERS
POTTS_RECORD_WORDS = 9     # TSU_POTTS_RECORD_WORDS
POTTS_MAX_Q = 8            # TSU_POTTS_MAX_Q
POTTS_HEAT_BATH, POTTS_SWENDSEN_WANG = 0, 1
POTTS_ROUTES = ("k10_small", "k10_sweep", "k10_sw_small", "k10_sw_tiles")  # TSU_POTTS_ROUTE_*
POTTS3D_ROUTES = ("k10_3d_small", "k10_3d_sweep", "k10_3d_sw_small", "k10_3d_sw_tiles")  # TSU_POTTS3D_ROUTE_*
CLUSTER_RECORD_WORDS = 8   # TSU_CLUSTER_RECORD_WORDS
CLUSTER_RECORD_FIELDS = ("n_clusters", "largest", "sum_size2", "sum_m2", "sum_m4", "n_frozen", "m_frozen")
MSC_SNAPSHOT_SLOTS = 8     # TSU_MSC_SNAPSHOT_SLOTS
MSC_C4_MAX_AXIS = 16382    # TSU_MSC_C4_MAX_AXIS

_lib = None


def load_library():
    """dlopen libtsu_hip.so and declare every prototype.  Raises HipUnavailableError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipUnavailableError(
            f"{LIB_PATH} not found: build it with tsu-emulator_amd/csrc/build.sh (hipcc, gfx950). "
            "This package has no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise HipUnavailableError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in (list(SIGNATURES.items()) + list(CLUSTER3D_SIGNATURES.items()) + list(CORRELATION_SIGNATURES.items())
                              + list(POPULATION_SIGNATURES.items()) + list(OVERLAP_SIGNATURES.items())
                              + list(ENSEMBLE_SIGNATURES.items()) + list(SPARSE_BATCH_SIGNATURES.items())
                              + list(PROBE_SIGNATURES.items()) + list(CLUSTER_FIELD_SIGNATURES.items())
                              + list(MULTISPIN_SIGNATURES.items()) + list(MULTISPIN_PT_SIGNATURES.items())
                              + list(MULTISPIN_CORR_SIGNATURES.items()) + list(MULTISPIN_QUENCH_SIGNATURES.items())
                              + list(CLUSTER_MEASURE_SIGNATURES.items()) + list(POTTS_SIGNATURES.items())
                              + list(POTTS3D_SIGNATURES.items()) + list(POTTS_MUCA_SIGNATURES.items())
                              + list(POTTS_DISORDER_SIGNATURES.items()) + list(POTTS_PT_SIGNATURES.items())
                              + list(POTTS_POP_SIGNATURES.items())):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(t)


REPLICA_LIMIT = 1 << 24  # TSU_REPLICA_LIMIT: a replica id shares its Philox counter word with the 8-bit stream tag


def _uint(name, value, bits):
    """``value`` as an int that fits an unsigned C integer of ``bits`` bits; ValueError otherwise (ctypes would wrap it silently)."""
    v = int(value)
    if not 0 <= v < (1 << bits):
        raise ValueError(f"{name} = {v} does not fit an unsigned {bits}-bit integer")
    return v


def _seed(seed):
    return _uint("seed", seed, 64)


def _counter(name, value):
    """A sweep0 / step0 / chain0 argument: a uint32 of the C ABI."""
    return _uint(name, value, 32)


def _replica(replica):
    v = _uint("replica", replica, 32)
    if v >= REPLICA_LIMIT:
        raise ValueError(f"replica = {v} is not below 2^24")
    return v


def _uint_array(name, values, dtype, limit=None):
    """Per-lattice / per-replica seeds, counters and replica ids as a contiguous unsigned array, range-checked first."""
    bits = 8 * np.dtype(dtype).itemsize
    vals = [_uint(name, v, bits) for v in np.asarray(values, dtype=object).ravel()]
    if limit is not None and any(v >= limit for v in vals):
        raise ValueError(f"{name}: every value must be below {limit}")
    return np.array(vals, dtype=dtype)


_live_contexts = weakref.WeakSet()


@atexit.register
def _shutdown_contexts():
    """Deterministic teardown at interpreter exit (before the HIP runtime's own exit handlers): every context still
    alive is synchronised and its streams / events are destroyed (``__del__`` is not reliable at finalisation)."""
    for ctx in list(_live_contexts):
        try:
            if getattr(ctx, "h", None):
                ctx.lib.tsu_shutdown(ctx.h)
                ctx.h = None
        except Exception:
            pass


class Context:
    """One tsu_ctx (one GPU).  ``Context.default()`` is the per-process singleton used by the API layer."""

    _default = None

    def __init__(self, device=-1):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.tsu_init(int(device), C.byref(h))
        if rc != TSU_OK:
            msg = self.lib.tsu_last_error(None).decode()
            raise HipUnavailableError(f"tsu_init failed ({rc}): {msg}")
        self.h = h
        _live_contexts.add(self)

    @classmethod
    def default(cls):
        if cls._default is None:
            dev = int(os.environ.get("TSU_HIP_DEVICE", os.environ.get("LOCAL_RANK", "-1")))
            cls._default = cls(dev)
        return cls._default

    def check(self, rc):
        if rc == TSU_OK:
            return
        msg = self.lib.tsu_last_error(self.h).decode()
        if rc == TSU_E_INVALID:
            raise ValueError(msg)
        if rc == TSU_E_UNSUPPORTED:
            raise UnsupportedError(msg)
        if rc == TSU_E_NOMEM:
            raise MemoryError(msg)
        if rc == TSU_E_RCCL:
            raise HipError(f"RCCL: {msg}")
        raise HipError(f"libtsu_hip error {rc}: {msg}")

    def set_stream(self, stream_ptr):
        self.check(self.lib.tsu_set_stream(self.h, _vp(stream_ptr or 0)))

    def synchronize(self):
        self.check(self.lib.tsu_synchronize(self.h))

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(0), C.c_uint64(0)
        self.check(self.lib.tsu_device_info(self.h, name, 256, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": mem.value}

    def timer_begin(self):
        self.check(self.lib.tsu_timer_begin(self.h))

    def timer_end(self):
        ms = C.c_float(0)
        self.check(self.lib.tsu_timer_end(self.h, C.byref(ms)))
        return ms.value

    def philox4x32_10(self, ctrs, key):
        ctrs = np.ascontiguousarray(ctrs, dtype=np.uint32).reshape(-1, 4)
        key = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
        out = np.zeros_like(ctrs)
        self.check(self.lib.tsu_philox4x32_10(self.h, ctrs.shape[0], _ptr(ctrs, _u32p), _ptr(key, _u32p),
                                              _ptr(out, _u32p)))
        return out

    def __del__(self, _finalizing=sys.is_finalizing):
        try:
            if getattr(self, "h", None) and not _finalizing():
                self.lib.tsu_shutdown(self.h)
                self.h = None
        except Exception:
            pass


def ising2d_thresholds(J, h, T, mode=MODE_PHYSICAL):
    """Host helper of the library (no GPU needed): table[deg*5+up] as uint64."""
    lib = load_library()
    t = np.zeros(25, dtype=np.uint64)
    rc = lib.tsu_ising2d_thresholds(float(J), float(h), float(T), int(mode), _ptr(t, _u64p))
    if rc != TSU_OK:
        raise ValueError("Temperature must be positive" if not T > 0 else "invalid threshold arguments")
    return t


def probe_screen(f32, a32, c32, ctx=None):
    """(t, m) of the K7 / K8 screen as the device computes them (tsu_probe_screen): float32 arrays of the inputs' common shape."""
    ctx = ctx or Context.default()
    f, a, c = (np.ascontiguousarray(v, dtype=np.float32) for v in np.broadcast_arrays(f32, a32, c32))
    t, m = np.empty_like(f), np.empty_like(f)
    ctx.check(ctx.lib.tsu_probe_screen(ctx.h, f.size, _ptr(f, _f32p), _ptr(a, _f32p), _ptr(c, _f32p), _ptr(t, _f32p), _ptr(m, _f32p)))
    return t, m


def _cluster_record(lat, entry):
    """The rows of a lattice's most recent measured cluster call as a dict of arrays over its steps (tsu_hip_cluster_measure.h):
    int64 arrays, ``sum_m4`` an object array of Python ints joined from its two words."""
    n = C.c_int(0)
    lat.ctx.check(entry(lat.h, None, 0, C.byref(n)))
    rows = np.zeros((n.value, CLUSTER_RECORD_WORDS), np.int64)
    if n.value:
        lat.ctx.check(entry(lat.h, _ptr(rows, _i64p), n.value, C.byref(n)))
    return cluster_record_dict(rows)


def cluster_record_dict(rows):
    """(n_steps, 8) int64 rows -> the dict of ``cluster_record()``; the two words of ``sum_m4`` are read as unsigned."""
    rows = np.asarray(rows, np.int64).reshape(-1, CLUSTER_RECORD_WORDS)
    out = {"n_clusters": rows[:, 0].copy(), "largest": rows[:, 1].copy(), "sum_size2": rows[:, 2].copy(), "sum_m2": rows[:, 3].copy()}
    m4 = np.empty(len(rows), object)
    for i, (lo, hi) in enumerate(rows[:, 4:6].astype(np.uint64).tolist()):
        m4[i] = (int(hi) << 64) | int(lo)
    out["sum_m4"] = m4
    out["n_frozen"] = rows[:, 6].copy()
    out["m_frozen"] = rows[:, 7].copy()
    return out


def cluster_threshold(J, T):
    """Host helper of the library (no GPU needed): the Swendsen-Wang bond threshold floor(p 2^32), p = -expm1(-2|J|/T)."""
    lib = load_library()
    t = C.c_uint64(0)
    rc = lib.tsu_ising2d_cluster_threshold(float(J), float(T), C.byref(t))
    if rc != TSU_OK:
        raise ValueError("Temperature must be positive" if not T > 0 else "invalid cluster threshold arguments")
    return t.value


class Lattice:
    """tsu_ising2d handle: a rows x cols lattice (or a row slab of one) of +-1 int8 spins on the GPU."""

    def __init__(self, rows, cols, periodic=False, ctx=None, total_rows=None, row0=0, ghost=0):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.rows, self.cols, self.periodic = int(rows), int(cols), bool(periodic)
        self.total_rows = int(total_rows if total_rows is not None else rows)
        self.row0, self.ghost = int(row0), int(ghost)
        h = _vp()
        self.ctx.check(self.lib.tsu_ising2d_create_slab(self.ctx.h, self.total_rows, self.cols, int(self.periodic),
                                                        self.row0, self.rows, self.ghost, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_ising2d_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():  # at interpreter exit the process teardown frees the device memory
            self.close()

    def set_spins(self, spins, row_first=0):
        s = np.ascontiguousarray(spins, dtype=np.int8).reshape(-1, self.cols)
        self.ctx.check(self.lib.tsu_ising2d_set_spins(self.h, _ptr(s, _i8p), int(row_first), s.shape[0]))

    def get_spins(self, row_first=0, n_rows=None):
        n_rows = self.rows if n_rows is None else int(n_rows)
        out = np.empty((n_rows, self.cols), dtype=np.int8)
        self.ctx.check(self.lib.tsu_ising2d_get_spins(self.h, _ptr(out, _i8p), int(row_first), n_rows))
        return out

    def randomize(self, seed, replica=0):
        self.ctx.check(self.lib.tsu_ising2d_randomize(self.h, _seed(seed), _replica(replica)))

    def fill(self, value):
        self.ctx.check(self.lib.tsu_ising2d_fill(self.h, int(value)))

    def set_thresholds(self, table):
        t = np.ascontiguousarray(table, dtype=np.uint64)
        if t.size != 25:
            raise ValueError("threshold table must have 25 entries")
        self.ctx.check(self.lib.tsu_ising2d_set_thresholds(self.h, _ptr(t, _u64p)))

    def set_model(self, J, h, T, mode=MODE_PHYSICAL):
        self.ctx.check(self.lib.tsu_ising2d_set_model(self.h, float(J), float(h), float(T), int(mode)))

    def set_kernel(self, kernel=KERNEL_AUTO, sweeps_per_launch=0):
        self.ctx.check(self.lib.tsu_ising2d_set_kernel(self.h, int(kernel), int(sweeps_per_launch)))

    def sweep(self, n_sweeps, seed, sweep0=0, replica=0):
        self.ctx.check(self.lib.tsu_ising2d_sweep(self.h, int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica)))

    def sweep_part(self, n_sweeps, seed, sweep0, part, replica=0):
        self.ctx.check(self.lib.tsu_ising2d_sweep_part(self.h, int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica), int(part)))

    def sample(self, n_burnin, n_sweeps, n_samples, seed, sweep0=0, replica=0):
        """n_burnin sweeps, then n_samples x (n_sweeps sweeps, record): (n_samples, rows, cols) int8, one PCIe transfer."""
        out = np.empty((int(n_samples), self.rows, self.cols), dtype=np.int8)
        self.ctx.check(self.lib.tsu_ising2d_sample(self.h, int(n_burnin), int(n_sweeps), int(n_samples), _seed(seed), _counter("sweep0", sweep0),
                                                   _replica(replica), _ptr(out, _i8p)))
        return out

    def observables(self):
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.tsu_ising2d_observables(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def row_ptr(self, local_row):
        p, pitch = _vp(), C.c_size_t(0)
        self.ctx.check(self.lib.tsu_ising2d_row_ptr(self.h, int(local_row), C.byref(p), C.byref(pitch)))
        return p.value, pitch.value

    def set_timing(self, enable=True):
        self.ctx.check(self.lib.tsu_ising2d_set_timing(self.h, int(bool(enable))))

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_ising2d_launch_count(self.h, C.byref(n)))
        return n.value

    def strip_numbering(self):
        """(generation, restarts) of the tile-resident kernel's strip numbering: generations numbered so far in the running
        numbering, and how often a numbering started over a cleared strip buffer (read-only)."""
        g, r = C.c_uint32(0), C.c_uint64(0)
        self.ctx.check(self.lib.tsu_ising2d_strip_numbering(self.h, C.byref(g), C.byref(r)))
        return g.value, r.value

    def last_sweep_ms(self):
        ms = C.c_float(0)
        self.ctx.check(self.lib.tsu_ising2d_last_sweep_ms(self.h, C.byref(ms)))
        return ms.value

    def cluster_sweep(self, J, T, n_steps, seed, step0=0, replica=0):
        """n_steps Swendsen-Wang steps at coupling J, temperature T, zero field (step counters step0 ..)."""
        self.ctx.check(self.lib.tsu_ising2d_cluster_sweep(self.h, float(J), float(T), int(n_steps), _seed(seed), _counter("step0", step0),
                                                          _replica(replica)))

    def cluster_launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_ising2d_cluster_launch_count(self.h, C.byref(n)))
        return n.value

    def cluster_measure(self, on=True):
        """The switch of the cluster-size records: while on, every cluster call records one row per step (same spins as off)."""
        self.ctx.check(self.lib.tsu_ising2d_cluster_measure(self.h, 1 if on else 0))

    def cluster_record(self):
        """The rows of the most recent measured cluster call (synchronises): a dict of arrays over its steps."""
        return _cluster_record(self, self.lib.tsu_ising2d_cluster_record)

    def set_disorder(self, J_right, J_down, h=None):
        """K7 quenched disorder: (rows, cols) arrays, rounded once to fp32 (h=None: zero field)."""
        shape = (self.rows, self.cols)
        jr = np.ascontiguousarray(J_right, dtype=np.float32).reshape(shape)
        jd = np.ascontiguousarray(J_down, dtype=np.float32).reshape(shape)
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(shape)
        self.ctx.check(self.lib.tsu_ising2d_set_disorder(self.h, _ptr(jr, _f32p), _ptr(jd, _f32p),
                                                         None if hh is None else _ptr(hh, _f32p)))

    def clear_disorder(self):
        self.ctx.check(self.lib.tsu_ising2d_clear_disorder(self.h))

    def disorder_sweep(self, T, n_sweeps, seed, sweep0=0, replica=0):
        """n_sweeps K7 heat-bath sweeps at temperature T (sweep counters sweep0 ..), K1's site uniforms."""
        self.ctx.check(self.lib.tsu_ising2d_disorder_sweep(self.h, float(T), int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica)))

    def disorder_energy(self):
        e = C.c_double(0)
        self.ctx.check(self.lib.tsu_ising2d_disorder_energy(self.h, C.byref(e)))
        return e.value

    def overlap(self, other):
        """sum_i s_i s'_i with another lattice of the same shape."""
        q = C.c_int64(0)
        self.ctx.check(self.lib.tsu_ising2d_overlap(self.h, other.h, C.byref(q)))
        return q.value

    def link_overlap(self, other):
        """(L, N_b): L = sum over the energy's bonds (i, j) of s_i s'_i s_j s'_j with another lattice of the same shape, and the
        number of those bonds."""
        L, nb = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.tsu_ising2d_link_overlap(self.h, other.h, C.byref(L), C.byref(nb)))
        return L.value, nb.value

    def disorder_launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_ising2d_disorder_launch_count(self.h, C.byref(n)))
        return n.value

    def profiles(self, other=None):
        """(P_row, P_col): exact int64 sums of s (or of s s' with another lattice of the same shape) over the columns / rows."""
        pr, pc = np.zeros(self.rows, np.int64), np.zeros(self.cols, np.int64)
        self.ctx.check(self.lib.tsu_ising2d_profiles(self.h, None if other is None else other.h, _ptr(pr, _i64p), _ptr(pc, _i64p)))
        return pr, pc


def _potts_tables(prefix, nb, q, J, h, T):
    """(E[0 .. nb], F[0 .. q - 1]) of the heat-bath rule with nb neighbours, from tsu_<prefix>_check_model."""
    lib = load_library()
    hh = None if h is None else np.ascontiguousarray(h, dtype=np.float64)
    if hh is not None and hh.shape != (int(q),) and 2 <= int(q) <= POTTS_MAX_Q:
        raise ValueError(f"h must hold q = {int(q)} values")
    t = np.zeros(nb + 1 + POTTS_MAX_Q, np.float64)
    rc = getattr(lib, f"tsu_{prefix}_check_model")(int(q), float(J), None if hh is None else _ptr(hh, _f64p), float(T), _ptr(t, _f64p))
    if rc != TSU_OK:
        raise ValueError("the Potts model (q, J, h, T) is refused: q outside 2 .. 8, a non-finite value, T <= 0 or "
                         f"({nb} |J| + max h - min h) / T > 600")
    return t[:nb + 1].copy(), t[nb + 1:nb + 1 + int(q)].copy()


def potts_tables(q, J, h, T):
    """Host helper of the library (no GPU needed): (E[0 .. 4], F[0 .. q - 1]) of the Potts heat-bath rule, or ValueError with the
    model refused (tsu_potts2d_check_model)."""
    return _potts_tables("potts2d", 4, q, J, h, T)


def potts3d_tables(q, J, h, T):
    """Host helper of the library (no GPU needed): (E[0 .. 6], F[0 .. q - 1]) of the six-neighbour Potts heat-bath rule, or ValueError
    with the model refused (tsu_potts3d_check_model)."""
    return _potts_tables("potts3d", 6, q, J, h, T)


def potts_cluster_threshold(J, T):
    """Host helper of the library (no GPU needed): the Potts bond threshold floor(-expm1(-J / T) 2^32)."""
    lib = load_library()
    t = C.c_uint64(0)
    if lib.tsu_potts2d_cluster_threshold(float(J), float(T), C.byref(t)) != TSU_OK:
        raise ValueError("the Potts cluster threshold needs finite J > 0 and T > 0")
    return t.value


def periodic_axes(periodic):
    """(p_z, p_r, p_c) from a bool (all three axes) or a triple of bools."""
    if isinstance(periodic, (bool, np.bool_)):
        return (bool(periodic),) * 3
    p = tuple(bool(x) for x in periodic)
    if len(p) != 3:
        raise ValueError("periodic must be a bool or a triple (p_z, p_r, p_c)")
    return p


class _PottsHandle:
    """What the two K10 handles share: every call but the constructor.  A subclass sets _prefix (the C symbols are
    tsu_<prefix>_<call>) and _routes, and its constructor sets q and shape and creates the handle through _create."""

    def _call(self, name, *args):
        self.ctx.check(getattr(self.lib, f"tsu_{self._prefix}_{name}")(*args))

    def _create(self, ctx, *args):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        h = _vp()
        self._call("create", self.ctx.h, *args, C.byref(h))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, f"tsu_{self._prefix}_destroy")(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def set_model(self, J, h=None):
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.float64)
        if hh is not None and hh.shape != (self.q,):
            raise ValueError(f"h must hold q = {self.q} values")
        self._call("set_model", self.h, float(J), None if hh is None else _ptr(hh, _f64p))

    def set_spins(self, colours):
        s = np.ascontiguousarray(colours, dtype=np.int8)
        if s.size != int(np.prod(self.shape)):
            raise ValueError("colours must hold " + " x ".join(str(n) for n in self.shape) + " values")
        self._call("set_spins", self.h, _ptr(s, _i8p))

    def get_spins(self):
        out = np.empty(self.shape, dtype=np.int8)
        self._call("get_spins", self.h, _ptr(out, _i8p))
        return out

    def fill(self, colour):
        self._call("fill", self.h, int(colour))

    def sweep(self, T, n_sweeps, seed, sweep0=0, replica=0):
        self._call("sweep", self.h, float(T), int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica))

    def cluster_sweep(self, T, n_steps, seed, step0=0, replica=0):
        self._call("cluster_sweep", self.h, float(T), int(n_steps), _seed(seed), _counter("step0", step0), _replica(replica))

    def route(self, algorithm=POTTS_HEAT_BATH):
        r = C.c_int(-1)
        self._call("route", self.h, int(algorithm), C.byref(r))
        return self._routes[r.value]

    def measure(self):
        """(n_eq, N_0 .. N_{q-1}) of the current state as exact integers (synchronises)."""
        row = np.zeros(POTTS_RECORD_WORDS, np.int64)
        self._call("measure", self.h, _ptr(row, _i64p))
        return int(row[0]), row[1:1 + self.q].copy()

    def run(self, T, n_meas, sweeps_between, algorithm, seed, counter0=0, replica=0):
        self._call("run", self.h, float(T), int(n_meas), int(sweeps_between), int(algorithm), _seed(seed), _counter("counter0", counter0),
                   _replica(replica))

    def record(self):
        """The rows of the most recent run (synchronises): (n_meas, 9) int64, n_eq then N_0 .. N_7."""
        n = C.c_int(0)
        self._call("record", self.h, None, 0, C.byref(n))
        rows = np.zeros((n.value, POTTS_RECORD_WORDS), np.int64)
        if n.value:
            self._call("record", self.h, _ptr(rows, _i64p), n.value, C.byref(n))
        return rows

    def launch_count(self):
        n = C.c_uint64(0)
        self._call("launch_count", self.h, C.byref(n))
        return n.value


class PottsLattice(_PottsHandle):
    """tsu_potts2d handle: a rows x cols lattice of colours 0 .. q - 1 (int8) on the GPU (K10)."""
    _prefix, _routes = "potts2d", POTTS_ROUTES

    def __init__(self, rows, cols, q, periodic=True, ctx=None):
        self.rows, self.cols, self.q, self.periodic = int(rows), int(cols), int(q), bool(periodic)
        self.shape = (self.rows, self.cols)
        self._create(ctx, self.rows, self.cols, self.q, int(self.periodic))


class PottsLattice3D(_PottsHandle):
    """tsu_potts3d handle: a depth x rows x cols lattice of colours 0 .. q - 1 (int8) on the GPU (K10 in 3-D); periodic is a bool
    (all three axes) or (p_z, p_r, p_c)."""
    _prefix, _routes = "potts3d", POTTS3D_ROUTES

    def __init__(self, depth, rows, cols, q, periodic=True, ctx=None):
        self.depth, self.rows, self.cols, self.q = int(depth), int(rows), int(cols), int(q)
        self.periodic = periodic_axes(periodic)
        self.shape = (self.depth, self.rows, self.cols)
        self._create(ctx, self.depth, self.rows, self.cols, self.q, *(int(x) for x in self.periodic))


def potts_site_thresholds(a, T):
    """Host helper of the library (no GPU needed): steps 2 - 5 of K12's heat-bath rule for one site, the integer thresholds
    thr[0 .. q - 1] of the sums a[0 .. q - 1] at temperature T (tsu_potts_dis_site_thresholds)."""
    lib = load_library()
    aa = np.ascontiguousarray(a, dtype=np.float64).ravel()
    thr = np.zeros(aa.size, np.uint64)
    if lib.tsu_potts_dis_site_thresholds(int(aa.size), _ptr(aa, _f64p), float(T), _ptr(thr, _u64p)) != TSU_OK:
        raise ValueError("the site is refused: q outside 2 .. 8, a non-finite sum or T, or T <= 0")
    return thr


class PottsDisorderLattice(_PottsHandle):
    """tsu_potts_dis handle (K12): a depth x rows x cols lattice of colours 0 .. q - 1 with per-bond couplings and a per-site colour
    field; shape (rows, cols) gives the 2-D lattice (depth 1, open z).  The arrays are checked and rounded to fp32 by the caller
    (tsu.models.potts); ``h`` is colour-major, (q,) + shape."""
    _prefix, _routes = "potts_dis", POTTS_DIS_ROUTES

    def __init__(self, shape, q, periodic=True, ctx=None):
        self.shape = tuple(int(n) for n in shape)
        self.q = int(q)
        dims = (1,) + self.shape if len(self.shape) == 2 else self.shape
        if len(self.shape) == 2:
            self.periodic = (False, bool(periodic), bool(periodic))
        else:
            self.periodic = periodic_axes(periodic)
        per = np.array([int(x) for x in self.periodic], np.int32)
        self._create(ctx, *dims, self.q, _ptr(per, _i32p))

    def set_disorder(self, J_right, J_down, J_layer=None, h=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (J_right, J_down, J_layer, h)]
        for a, want in zip(arrs, (self.shape, self.shape, self.shape, (self.q,) + self.shape)):
            if a is not None and a.shape != want:
                raise ValueError(f"a disorder array has shape {a.shape}, expected {want}")
        self._call("set_disorder", self.h, *(None if a is None else _ptr(a, _f32p) for a in arrs))

    def measure(self):
        """(n_eq, N_0 .. N_{q-1}, E): exact integers and the float64 energy in the device's fixed order (synchronises)."""
        row = np.zeros(POTTS_RECORD_WORDS, np.int64)
        e = C.c_double(0.0)
        self._call("measure", self.h, _ptr(row, _i64p), C.byref(e))
        return int(row[0]), row[1:1 + self.q].copy(), e.value

    def record(self):
        """The rows of the most recent run (synchronises): ((n_meas, 9) int64: n_eq then N_0 .. N_7, (n_meas,) float64: E)."""
        n = C.c_int(0)
        self._call("record", self.h, None, 0, C.byref(n))
        rows = np.zeros((n.value, POTTS_DIS_RECORD_WORDS), np.int64)
        if n.value:
            self._call("record", self.h, _ptr(rows, _i64p), n.value, C.byref(n))
        return rows[:, :POTTS_RECORD_WORDS].copy(), rows[:, POTTS_RECORD_WORDS].copy().view(np.float64)


class PottsTemperingLattice:
    """tsu_potts_pt handle (K13 parallel tempering): n_ladders ladders of n_temps walkers of one K12 lattice sharing one disorder;
    shape (rows, cols) gives the 2-D lattice (depth 1, open z).  Walker w of ladder k has Philox key seed + k n_temps + w and
    starts at slot w.  The arrays are checked and rounded to fp32 by the caller (tsu.models.potts_tempering)."""

    def __init__(self, shape, q, periodic, n_temps, n_ladders=1, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.shape = tuple(int(n) for n in shape)
        self.q, self.n_temps, self.n_ladders = int(q), int(n_temps), int(n_ladders)
        dims = (1,) + self.shape if len(self.shape) == 2 else self.shape
        if len(self.shape) == 2:
            self.periodic = (False, bool(periodic), bool(periodic))
        else:
            self.periodic = periodic_axes(periodic)
        per = np.array([int(x) for x in self.periodic], np.int32)
        self._recorded = 0
        h = _vp()
        self.ctx.check(self.lib.tsu_potts_pt_create(self.ctx.h, *dims, self.q, _ptr(per, _i32p), self.n_temps, self.n_ladders, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_potts_pt_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def set_disorder(self, J_right, J_down, J_layer=None, h=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (J_right, J_down, J_layer, h)]
        for a, want in zip(arrs, (self.shape, self.shape, self.shape, (self.q,) + self.shape)):
            if a is not None and a.shape != want:
                raise ValueError(f"a disorder array has shape {a.shape}, expected {want}")
        self.ctx.check(self.lib.tsu_potts_pt_set_disorder(self.h, *(None if a is None else _ptr(a, _f32p) for a in arrs)))

    def set_temperatures(self, T):
        t = np.ascontiguousarray(T, dtype=np.float64).ravel()
        if t.size != self.n_temps:
            raise ValueError(f"need {self.n_temps} temperatures, got {t.size}")
        self.ctx.check(self.lib.tsu_potts_pt_set_temperatures(self.h, _ptr(t, _f64p)))

    def init(self, seed, initial=-1):
        """initial -1: the colours stay (set them with set_spins afterwards); a colour 0 .. q - 1: that colour everywhere."""
        self.ctx.check(self.lib.tsu_potts_pt_init(self.h, _seed(seed), int(initial)))
        self._recorded = 0

    def advance(self, n_sweeps):
        self.ctx.check(self.lib.tsu_potts_pt_advance(self.h, _uint("n_sweeps", n_sweeps, 64)))

    def run(self, n_rounds, swap_interval, swap=True, record=True):
        self._recorded = 0
        self.ctx.check(self.lib.tsu_potts_pt_run(self.h, int(n_rounds), int(swap_interval), int(bool(swap)), int(bool(record))))
        self._recorded = int(n_rounds) if record else 0

    def history(self):
        """The last run's rows: E, n_eq, walker as (n_rounds, n_ladders, n_temps); N as (.., q); tables (n_rounds, n_temps, q, q) or
        None with one ladder."""
        n, nl, R, q = self._recorded, self.n_ladders, self.n_temps, self.q
        E = np.zeros((n, nl, R))
        M = np.zeros((n, nl, R), np.int64)
        N = np.zeros((n, nl, R, POTTS_MAX_Q), np.int64)
        W = np.zeros((n, nl, R), np.int32)
        self.ctx.check(self.lib.tsu_potts_pt_history(self.h, _ptr(E, _f64p), _ptr(M, _i64p), _ptr(N, _i64p), _ptr(W, _i32p)))
        tables = None
        if nl == 2:
            tables = np.zeros((n, R, q, q), np.int64)
            self.ctx.check(self.lib.tsu_potts_pt_overlap_tables(self.h, _ptr(tables, _i64p)))
        return {"E": E, "n_eq": M, "N": N[..., :q].copy(), "walker": W, "tables": tables}

    def stats(self):
        nl, R = self.n_ladders, self.n_temps
        att, acc = np.zeros((nl, R - 1), np.int64), np.zeros((nl, R - 1), np.int64)
        trips, was = np.zeros((nl, R), np.int64), np.zeros((nl, R), np.int32)
        sw, rd = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self.lib.tsu_potts_pt_stats(self.h, _ptr(att, _i64p), _ptr(acc, _i64p), _ptr(trips, _i64p), _ptr(was, _i32p),
                                                   C.byref(sw), C.byref(rd)))
        return {"attempts": att, "accepts": acc, "round_trips": trips, "walker_at_slot": was, "sweep_count": sw.value,
                "round_count": rd.value}

    def energies(self):
        """(E, n_eq) of every walker now, as (n_ladders, n_temps) arrays indexed by walker."""
        E = np.zeros((self.n_ladders, self.n_temps))
        M = np.zeros((self.n_ladders, self.n_temps), np.int64)
        self.ctx.check(self.lib.tsu_potts_pt_energies(self.h, _ptr(E, _f64p), _ptr(M, _i64p)))
        return E, M

    def get_spins(self, ladder, slot):
        out = np.empty(self.shape, dtype=np.int8)
        self.ctx.check(self.lib.tsu_potts_pt_get_spins(self.h, int(ladder), int(slot), _ptr(out, _i8p)))
        return out

    def set_spins(self, ladder, slot, colours):
        s = np.ascontiguousarray(colours, dtype=np.int8).reshape(self.shape)
        self.ctx.check(self.lib.tsu_potts_pt_set_spins(self.h, int(ladder), int(slot), _ptr(s, _i8p)))

    def route(self):
        r = C.c_int(-1)
        self.ctx.check(self.lib.tsu_potts_pt_route(self.h, C.byref(r)))
        return POTTS_PT_ROUTES[r.value]

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_potts_pt_launch_count(self.h, C.byref(n)))
        return n.value


class PottsPopulation:
    """tsu_potts_pop handle (K14 population annealing): `population` walkers of one K12 lattice sharing one disorder; shape (rows,
    cols) gives the 2-D lattice (depth 1, open z).  Walker i has Philox key seed + i.  The arrays are checked and rounded to fp32 by
    the caller (tsu.models.potts_population)."""

    def __init__(self, shape, q, periodic, population, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.shape = tuple(int(n) for n in shape)
        self.q, self.population = int(q), int(population)
        dims = (1,) + self.shape if len(self.shape) == 2 else self.shape
        if len(self.shape) == 2:
            self.periodic = (False, bool(periodic), bool(periodic))
        else:
            self.periodic = periodic_axes(periodic)
        per = np.array([int(x) for x in self.periodic], np.int32)
        self._recorded = -1
        h = _vp()
        self.ctx.check(self.lib.tsu_potts_pop_create(self.ctx.h, *dims, self.q, _ptr(per, _i32p), self.population, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_potts_pop_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def set_disorder(self, J_right, J_down, J_layer=None, h=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (J_right, J_down, J_layer, h)]
        for a, want in zip(arrs, (self.shape, self.shape, self.shape, (self.q,) + self.shape)):
            if a is not None and a.shape != want:
                raise ValueError(f"a disorder array has shape {a.shape}, expected {want}")
        self.ctx.check(self.lib.tsu_potts_pop_set_disorder(self.h, *(None if a is None else _ptr(a, _f32p) for a in arrs)))

    def set_schedule(self, betas):
        b = np.ascontiguousarray(betas, dtype=np.float64).ravel()
        self.ctx.check(self.lib.tsu_potts_pop_set_schedule(self.h, _ptr(b, _f64p), int(b.size)))

    def init(self, seed, initial=POTTS_POP_DRAW, initial_sweeps=0):
        """initial -2: the device draw; -1: the colours stay (set_spins); a colour 0 .. q - 1: that colour everywhere."""
        self._recorded = -1
        self.ctx.check(self.lib.tsu_potts_pop_init(self.h, _seed(seed), int(initial), int(initial_sweeps)))

    def advance(self, n_sweeps):
        self.ctx.check(self.lib.tsu_potts_pop_advance(self.h, _uint("n_sweeps", n_sweeps, 64)))

    def run(self, n_steps, sweeps_per_step, resample=True, record=True):
        self._recorded = -1
        self.ctx.check(self.lib.tsu_potts_pop_run(self.h, int(n_steps), int(sweeps_per_step), int(bool(resample)), int(bool(record))))
        self._recorded = int(n_steps) if record else -1

    def history(self):
        """The last recording run's rows: E, n_eq (n + 1, R); N (n + 1, R, q); W, parent (n, R); S, U, E_min (n,)."""
        if self._recorded < 0:
            raise ValueError("potts_pop_history: the last run recorded nothing")
        n, R = self._recorded, self.population
        E, M = np.zeros((n + 1, R)), np.zeros((n + 1, R), np.int64)
        N = np.zeros((n + 1, R, POTTS_MAX_Q), np.int64)
        W, P = np.zeros((n, R), np.uint32), np.zeros((n, R), np.int32)
        S, U, Em = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n)
        self.ctx.check(self.lib.tsu_potts_pop_history(self.h, _ptr(E, _f64p), _ptr(M, _i64p), _ptr(N, _i64p), _ptr(W, _u32p), _ptr(P, _i32p),
                                                      _ptr(S, _u64p), _ptr(U, _u64p), _ptr(Em, _f64p)))
        return {"E": E, "n_eq": M, "N": N[..., :self.q].copy(), "W": W, "parent": P, "S": S, "U": U, "E_min": Em}

    def energies(self):
        """(E, n_eq) of every walker now."""
        E, M = np.zeros(self.population), np.zeros(self.population, np.int64)
        self.ctx.check(self.lib.tsu_potts_pop_energies(self.h, _ptr(E, _f64p), _ptr(M, _i64p)))
        return E, M

    def get_spins(self, i):
        out = np.empty(self.shape, dtype=np.int8)
        self.ctx.check(self.lib.tsu_potts_pop_get_spins(self.h, int(i), _ptr(out, _i8p)))
        return out

    def set_spins(self, i, colours):
        s = np.ascontiguousarray(colours, dtype=np.int8).reshape(self.shape)
        self.ctx.check(self.lib.tsu_potts_pop_set_spins(self.h, int(i), _ptr(s, _i8p)))

    def get_padded(self, i):
        """Walker i's slot of the allocation: the colours and the pad bytes, sites rounded up to a multiple of 16 in all."""
        out = np.empty((int(np.prod(self.shape)) + 15) // 16 * 16, dtype=np.int8)
        self.ctx.check(self.lib.tsu_potts_pop_get_padded(self.h, int(i), _ptr(out, _i8p)))
        return out

    def route(self):
        r = C.c_int(-1)
        self.ctx.check(self.lib.tsu_potts_pop_route(self.h, C.byref(r)))
        return POTTS_POP_ROUTES[r.value]

    def plan(self):
        """What the packing rule gives this handle now: route, walkers per workgroup, lanes per workgroup, LDS bytes."""
        r, g, t, b = C.c_int(-1), C.c_int(0), C.c_int(0), C.c_int(0)
        self.ctx.check(self.lib.tsu_potts_pop_plan(self.h, C.byref(r), C.byref(g), C.byref(t), C.byref(b)))
        return {"route": POTTS_POP_ROUTES[r.value], "G": g.value, "threads": t.value, "lds_bytes": b.value}

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_potts_pop_launch_count(self.h, C.byref(n)))
        return n.value


def potts_muca_geometry(depth, rows, cols, periodic):
    """Host helper of the library (no GPU needed): (B, z_max) of a depth x rows x cols lattice, ValueError where it is refused."""
    lib = load_library()
    per = np.array([int(bool(x)) for x in periodic_axes(periodic)], np.int32)
    b, z = C.c_int64(0), C.c_int(0)
    if lib.tsu_potts_muca_geometry(int(depth), int(rows), int(cols), _ptr(per, _i32p), C.byref(b), C.byref(z)) != TSU_OK:
        raise ValueError(f"a side < 1 or more than {POTTS_MUCA_MAX_SITES} sites")
    return b.value, z.value


def potts_muca_thresholds(bonds, z_max, lnw):
    """Host helper of the library (no GPU needed): the (B + 1, 2 z_max + 1) uint64 acceptance table of ln W, the one the device decides
    with (tsu_potts_muca_thresholds)."""
    lib = load_library()
    w = np.ascontiguousarray(lnw, dtype=np.float64)
    if w.shape != (int(bonds) + 1,):
        raise ValueError(f"lnw must hold B + 1 = {int(bonds) + 1} values")
    out = np.zeros((int(bonds) + 1, 2 * int(z_max) + 1), np.uint64)
    if lib.tsu_potts_muca_thresholds(int(bonds), int(z_max), _ptr(w, _f64p), _ptr(out, _u64p)) != TSU_OK:
        raise ValueError("the table is refused: B < 0, z_max other than 4 or 6, or a non-finite ln W")
    return out


class PottsMucaWalkers:
    """tsu_potts_muca handle (K11): `walkers` copies of a depth x rows x cols lattice of colours 0 .. q - 1 under one weight table
    ln W[n_eq], with the shared exact record H, S1, S2."""

    def __init__(self, depth, rows, cols, q, walkers, periodic=True, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.depth, self.rows, self.cols, self.q, self.walkers = int(depth), int(rows), int(cols), int(q), int(walkers)
        self.periodic = periodic_axes(periodic)
        per = np.array([int(x) for x in self.periodic], np.int32)
        h = _vp()
        self.ctx.check(self.lib.tsu_potts_muca_create(self.ctx.h, self.depth, self.rows, self.cols, self.q, _ptr(per, _i32p), self.walkers,
                                                      C.byref(h)))
        self.h = h
        self.bonds, self.z_max = potts_muca_geometry(self.depth, self.rows, self.cols, self.periodic)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_potts_muca_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def set_weights(self, lnw):
        w = np.ascontiguousarray(lnw, dtype=np.float64).ravel()
        self.ctx.check(self.lib.tsu_potts_muca_set_weights(self.h, _ptr(w, _f64p), w.size))

    def set_spins(self, colours):
        s = np.ascontiguousarray(colours, dtype=np.int8)
        if s.size != self.walkers * self.depth * self.rows * self.cols:
            raise ValueError(f"colours must hold {self.walkers} x {self.depth} x {self.rows} x {self.cols} values")
        self.ctx.check(self.lib.tsu_potts_muca_set_spins(self.h, _ptr(s, _i8p)))

    def get_spins(self):
        out = np.empty((self.walkers, self.depth, self.rows, self.cols), dtype=np.int8)
        self.ctx.check(self.lib.tsu_potts_muca_get_spins(self.h, _ptr(out, _i8p)))
        return out

    def fill(self, colour):
        self.ctx.check(self.lib.tsu_potts_muca_fill(self.h, int(colour)))

    def set_tunnel_bounds(self, n_lo, n_hi):
        self.ctx.check(self.lib.tsu_potts_muca_set_tunnel_bounds(self.h, int(n_lo), int(n_hi)))

    def run(self, n_sweeps, seed, sweep0=0, replica=0):
        self.ctx.check(self.lib.tsu_potts_muca_run(self.h, int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica)))

    def energies(self):
        out = np.empty(self.walkers, np.int32)
        self.ctx.check(self.lib.tsu_potts_muca_energies(self.h, _ptr(out, _i32p)))
        return out

    def tunnels(self):
        out = np.empty(self.walkers, np.uint32)
        self.ctx.check(self.lib.tsu_potts_muca_tunnels(self.h, _ptr(out, _u32p)))
        return out

    def record(self):
        """(H, S1, S2), B + 1 uint64 words each (synchronises)."""
        out = np.zeros((3, self.bonds + 1), np.uint64)
        self.ctx.check(self.lib.tsu_potts_muca_record(self.h, _ptr(out[0], _u64p), _ptr(out[1], _u64p), _ptr(out[2], _u64p)))
        return out[0], out[1], out[2]

    def clear_record(self):
        self.ctx.check(self.lib.tsu_potts_muca_clear_record(self.h))

    def measure(self):
        """Recomputes n_eq and N_c of every walker from the spins; True iff they equalled the incrementally kept ones."""
        eq = C.c_int(0)
        self.ctx.check(self.lib.tsu_potts_muca_measure(self.h, C.byref(eq)))
        return bool(eq.value)

    def route(self):
        r = C.c_int(-1)
        self.ctx.check(self.lib.tsu_potts_muca_route(self.h, C.byref(r)))
        return POTTS_MUCA_ROUTES[r.value]

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_potts_muca_launch_count(self.h, C.byref(n)))
        return n.value


class Lattice3D:
    """tsu_ising3d handle (K8): a depth x rows x cols lattice of +-1 int8 spins with per-bond couplings and per-site fields.
    ``periodic``: a bool or a triple (p_z, p_r, p_c)."""

    def __init__(self, depth, rows, cols, periodic=False, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.depth, self.rows, self.cols = int(depth), int(rows), int(cols)
        self.shape = (self.depth, self.rows, self.cols)
        self.periodic = periodic_axes(periodic)
        mask = sum(1 << a for a in range(3) if self.periodic[a])
        h = _vp()
        self.ctx.check(self.lib.tsu_ising3d_create(self.ctx.h, self.depth, self.rows, self.cols, mask, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_ising3d_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():  # at interpreter exit the process teardown frees the device memory
            self.close()

    def set_spins(self, spins):
        s = np.ascontiguousarray(spins, dtype=np.int8).reshape(self.shape)
        self.ctx.check(self.lib.tsu_ising3d_set_spins(self.h, _ptr(s, _i8p)))

    def get_spins(self):
        out = np.empty(self.shape, dtype=np.int8)
        self.ctx.check(self.lib.tsu_ising3d_get_spins(self.h, _ptr(out, _i8p)))
        return out

    def randomize(self, seed, replica=0):
        self.ctx.check(self.lib.tsu_ising3d_randomize(self.h, _seed(seed), _replica(replica)))

    def fill(self, value):
        self.ctx.check(self.lib.tsu_ising3d_fill(self.h, int(value)))

    def set_disorder(self, J_right, J_down, J_layer, h=None):
        """K8 quenched disorder: (depth, rows, cols) arrays, rounded once to fp32 (h=None: zero field)."""
        jr, jd, jl = (np.ascontiguousarray(a, dtype=np.float32).reshape(self.shape) for a in (J_right, J_down, J_layer))
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(self.shape)
        self.ctx.check(self.lib.tsu_ising3d_set_disorder(self.h, _ptr(jr, _f32p), _ptr(jd, _f32p), _ptr(jl, _f32p),
                                                         None if hh is None else _ptr(hh, _f32p)))

    def sweep(self, T, n_sweeps, seed, sweep0=0, replica=0):
        """n_sweeps K8 heat-bath sweeps at temperature T (sweep counters sweep0 ..)."""
        self.ctx.check(self.lib.tsu_ising3d_sweep(self.h, float(T), int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica)))

    def energy(self):
        e = C.c_double(0)
        self.ctx.check(self.lib.tsu_ising3d_energy(self.h, C.byref(e)))
        return e.value

    def sum_spins(self):
        m = C.c_int64(0)
        self.ctx.check(self.lib.tsu_ising3d_sum_spins(self.h, C.byref(m)))
        return m.value

    def overlap(self, other):
        """sum_i s_i s'_i with another lattice of the same shape."""
        q = C.c_int64(0)
        self.ctx.check(self.lib.tsu_ising3d_overlap(self.h, other.h, C.byref(q)))
        return q.value

    def link_overlap(self, other):
        """(L, N_b): L = sum over the energy's bonds (i, j) of s_i s'_i s_j s'_j with another lattice of the same shape, and the
        number of those bonds."""
        L, nb = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.tsu_ising3d_link_overlap(self.h, other.h, C.byref(L), C.byref(nb)))
        return L.value, nb.value

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_ising3d_launch_count(self.h, C.byref(n)))
        return n.value

    def profiles(self, other=None):
        """(P_z, P_r, P_c): exact int64 sums of s (or of s s' with another lattice of the same shape) over the other two axes."""
        out = tuple(np.zeros(n, np.int64) for n in self.shape)
        self.ctx.check(self.lib.tsu_ising3d_profiles(self.h, None if other is None else other.h, *[_ptr(a, _i64p) for a in out]))
        return out

    def cluster_sweep(self, T, n_steps, seed, step0=0, replica=0):
        """n_steps Swendsen-Wang steps on the stored couplings at temperature T, zero field (step counters step0 ..)."""
        self.ctx.check(self.lib.tsu_ising3d_cluster_sweep(self.h, float(T), int(n_steps), _seed(seed), _counter("step0", step0), _replica(replica)))

    def cluster_sweep_field(self, T, n_steps, seed, step0=0, replica=0):
        """n_steps ghost-spin Swendsen-Wang steps on the stored couplings and field at temperature T (step counters step0 ..); with
        zero field the spins of ``cluster_sweep``."""
        self.ctx.check(self.lib.tsu_ising3d_cluster_sweep_field(self.h, float(T), int(n_steps), _seed(seed), _counter("step0", step0), _replica(replica)))

    def cluster_launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_ising3d_cluster_launch_count(self.h, C.byref(n)))
        return n.value

    def cluster_measure(self, on=True):
        """The switch of the cluster-size records: while on, every cluster call, zero-field or ghost, records one row per step."""
        self.ctx.check(self.lib.tsu_ising3d_cluster_measure(self.h, 1 if on else 0))

    def cluster_record(self):
        """The rows of the most recent measured cluster call (synchronises): a dict of arrays over its steps."""
        return _cluster_record(self, self.lib.tsu_ising3d_cluster_record)


def msc_thresholds(T):
    """Host helper of the library (no GPU needed): K9's table[f + 6] for f = -6 .. 6 as uint64 (tsu_msc_thresholds)."""
    lib = load_library()
    t = np.zeros(13, dtype=np.uint64)
    if lib.tsu_msc_thresholds(float(T), _ptr(t, _u64p)) != TSU_OK:
        raise ValueError("Temperature must be positive")
    return t


def msc_pack(bits):
    """(S, ...) booleans -> (ceil(S / 64), ...) uint64: bit b of word-plane w is sample 64 w + b; pad bits 0."""
    bits = np.asarray(bits, dtype=bool)
    S, shape = bits.shape[0], bits.shape[1:]
    W = (S + 63) // 64
    padded = np.zeros((W * 64,) + shape, dtype=np.uint8)
    padded[:S] = bits
    by_word = np.moveaxis(padded.reshape((W, 64) + shape), 1, -1)
    return np.ascontiguousarray(np.packbits(by_word, axis=-1, bitorder="little")).view("<u8").reshape((W,) + shape)


def msc_unpack(words, n_samples):
    """(W, ...) uint64 -> (n_samples, ...) booleans, the inverse of :func:`msc_pack` (pad bits dropped)."""
    words = np.ascontiguousarray(words, dtype="<u8")
    W, shape = words.shape[0], words.shape[1:]
    by_word = np.unpackbits(words.view(np.uint8).reshape((W,) + shape + (8,)), axis=-1, bitorder="little")
    return np.moveaxis(by_word, -1, 1).reshape((W * 64,) + shape)[:int(n_samples)].astype(bool)


class MultispinLattice:
    """tsu_msc handle (K9): n_temps x replicas x ceil(n_samples / 64) planes of uint64, 64 samples of a +-1 glass per word."""

    def __init__(self, depth, rows, cols, periodic, n_temps, replicas, n_samples, route=MSC_ROUTE_AUTO, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.shape = (int(depth), int(rows), int(cols))
        self.periodic = periodic_axes(periodic)
        self.n_temps, self.replicas, self.n_samples = int(n_temps), int(replicas), int(n_samples)
        self.words = (self.n_samples + 63) // 64
        mask = sum(1 << a for a in range(3) if self.periodic[a])
        h = _vp()
        self.ctx.check(self.lib.tsu_msc_create(self.ctx.h, *self.shape, mask, self.n_temps, self.replicas, self.n_samples, int(route),
                                               C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_msc_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    @property
    def route(self):
        r = C.c_int(0)
        self.ctx.check(self.lib.tsu_msc_route(self.h, C.byref(r)))
        return r.value

    def set_couplings(self, J_right, J_down, J_layer):
        """Packed couplings, (words, depth, rows, cols) uint64 each; a set bit is J = -1."""
        a = [np.ascontiguousarray(x, dtype=np.uint64).reshape((self.words,) + self.shape) for x in (J_right, J_down, J_layer)]
        self.ctx.check(self.lib.tsu_msc_set_couplings(self.h, *(_ptr(x, _u64p) for x in a)))

    def _plane_shape(self):
        return (self.n_temps, self.replicas, self.words) + self.shape

    def set_planes(self, planes):
        p = np.ascontiguousarray(planes, dtype=np.uint64).reshape(self._plane_shape())
        self.ctx.check(self.lib.tsu_msc_set_planes(self.h, _ptr(p, _u64p)))

    def get_planes(self):
        out = np.empty(self._plane_shape(), dtype=np.uint64)
        self.ctx.check(self.lib.tsu_msc_get_planes(self.h, _ptr(out, _u64p)))
        return out

    def set_seeds(self, seeds):
        s = _uint_array("seeds", seeds, np.uint64)
        if s.size != self.n_temps * self.replicas:
            raise ValueError(f"seeds must hold n_temps x replicas = {self.n_temps * self.replicas} values, got {s.size}")
        self.ctx.check(self.lib.tsu_msc_set_seeds(self.h, _ptr(s, _u64p)))

    def randomize(self):
        self.ctx.check(self.lib.tsu_msc_randomize(self.h))

    def fill(self, value):
        self.ctx.check(self.lib.tsu_msc_fill(self.h, int(value)))

    def set_temperatures(self, T):
        t = np.ascontiguousarray(T, dtype=np.float64).ravel()
        if t.size != self.n_temps:
            raise ValueError(f"expected {self.n_temps} temperatures, got {t.size}")
        self.ctx.check(self.lib.tsu_msc_set_temperatures(self.h, _ptr(t, _f64p)))

    def sweep(self, n_sweeps, sweep0=0):
        self.ctx.check(self.lib.tsu_msc_sweep(self.h, int(n_sweeps), _counter("sweep0", sweep0)))

    def measure(self):
        """(unsat, sum, q, q_link): int64 arrays (n_temps, replicas, S), (n_temps, replicas, S), and with two replicas
        (n_temps, S) each (else None); pad columns dropped."""
        cols = self.words * 64
        unsat = np.zeros((self.n_temps, self.replicas, cols), np.int64)
        ssum = np.zeros_like(unsat)
        two = self.replicas == 2
        q = np.zeros((self.n_temps, cols), np.int64) if two else None
        ql = np.zeros((self.n_temps, cols), np.int64) if two else None
        self.ctx.check(self.lib.tsu_msc_measure(self.h, _ptr(unsat, _i64p), _ptr(ssum, _i64p), _ptr(q, _i64p) if two else None,
                                                _ptr(ql, _i64p) if two else None))
        S = self.n_samples
        return (unsat[..., :S].copy(), ssum[..., :S].copy(), q[..., :S].copy() if two else None, ql[..., :S].copy() if two else None)

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_msc_launch_count(self.h, C.byref(n)))
        return n.value

    # ---- tempering (tsu_msc_pt_*): per-sample swaps between the temperature slots, decided and applied on the device
    def pt_enable(self, T):
        t = np.ascontiguousarray(T, dtype=np.float64).ravel()
        if t.size != self.n_temps:
            raise ValueError(f"expected {self.n_temps} temperatures, got {t.size}")
        self.ctx.check(self.lib.tsu_msc_pt_enable(self.h, _ptr(t, _f64p)))

    def pt_set_swap_seeds(self, seeds):
        s = _uint_array("swap_seeds", seeds, np.uint64)
        if s.size != self.n_samples:
            raise ValueError(f"swap_seeds must hold one value per sample ({self.n_samples}), got {s.size}")
        self.ctx.check(self.lib.tsu_msc_pt_set_swap_seeds(self.h, _ptr(s, _u64p)))

    def pt_run(self, n_rounds, swap_interval, swap=True, record=True, sweep0=0, round0=0):
        # a run that ended exactly at a limit leaves round0 = 2^32, which no uint32 carries to the library's own check: refuse
        # here in its words and its order (the sweep counter first)
        if int(n_rounds) > 0 and int(swap_interval) >= 0:
            if int(sweep0) + int(n_rounds) * int(swap_interval) > 1 << 31:
                raise ValueError("msc_pt_run: sweep counter overflow")
            if int(round0) + int(n_rounds) > 1 << 32:
                raise ValueError("msc_pt_run: round counter overflow")
        self.ctx.check(self.lib.tsu_msc_pt_run(self.h, int(n_rounds), int(swap_interval), int(bool(swap)), int(bool(record)),
                                               _counter("sweep0", sweep0), _counter("round0", round0)))

    def pt_stats(self):
        """attempts, accepts (replicas, S, n_temps - 1) and labels, flags, trips (replicas, S, n_temps) of the swap passes so far."""
        A, S, R = self.replicas, self.n_samples, self.n_temps
        att = np.zeros((A, S, R - 1), np.int64)
        acc = np.zeros_like(att)
        lab = np.zeros((A, S, R), np.int32)
        flg = np.zeros_like(lab)
        trips = np.zeros((A, S, R), np.int64)
        self.ctx.check(self.lib.tsu_msc_pt_stats(self.h, _ptr(att, _i64p), _ptr(acc, _i64p), _ptr(lab, _i32p), _ptr(flg, _i32p),
                                                 _ptr(trips, _i64p)))
        return {"attempts": att, "accepts": acc, "label_at_slot": lab, "flags": flg, "round_trips": trips}

    def pt_history(self, n_rows):
        """The rows the last ``pt_run`` recorded, each as :meth:`measure` gives it: (unsat, sum, q, q_link) with a leading round axis."""
        n, cols = int(n_rows), self.words * 64
        unsat = np.zeros((n, self.n_temps, self.replicas, cols), np.int64)
        ssum = np.zeros_like(unsat)
        two = self.replicas == 2
        q = np.zeros((n, self.n_temps, cols), np.int64) if two else None
        ql = np.zeros((n, self.n_temps, cols), np.int64) if two else None
        self.ctx.check(self.lib.tsu_msc_pt_history(self.h, n, _ptr(unsat, _i64p), _ptr(ssum, _i64p), _ptr(q, _i64p) if two else None,
                                                   _ptr(ql, _i64p) if two else None))
        S = self.n_samples
        return (unsat[..., :S].copy(), ssum[..., :S].copy(), q[..., :S].copy() if two else None, ql[..., :S].copy() if two else None)

    def pt_launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_msc_pt_launch_count(self.h, C.byref(n)))
        return n.value

    # ---- correlation (tsu_msc_profiles / _set_correlation / _modes / _pt_history_modes): axis profiles and k_min modes
    def profiles(self):
        """(P_z, P_r, P_c): int64 (n_temps, S, L_d) profiles of a * b (two replicas) or of the spins (one); pad columns dropped."""
        cols, S = self.words * 64, self.n_samples
        out = [np.zeros((self.n_temps, cols, n), np.int64) for n in self.shape]
        self.ctx.check(self.lib.tsu_msc_profiles(self.h, *(_ptr(x, _i64p) for x in out)))
        return tuple(x[:, :S].copy() for x in out)

    def set_correlation(self, tables):
        """``tables``: per axis (cos, sin) float64 arrays of the axis's length, or None for an open axis; ``None`` switches the
        modes off."""
        if tables is None:
            self.ctx.check(self.lib.tsu_msc_set_correlation(self.h, 0, None, None, None, None, None, None))
            self._mode_axes = None
            return
        if len(tables) != 3:
            raise ValueError("set_correlation: one (cos, sin) pair or None per axis (depth, rows, cols)")
        keep, args = [], []
        for n, t in zip(self.shape, tables):
            if t is None:
                args += [None, None]
                continue
            pair = [np.ascontiguousarray(x, dtype=np.float64).ravel() for x in t]
            if len(pair) != 2 or any(x.size != n for x in pair):
                raise ValueError(f"set_correlation: the tables of an axis of length {n} must be two arrays of that length")
            keep += pair
            args += [_ptr(x, _f64p) for x in pair]
        self.ctx.check(self.lib.tsu_msc_set_correlation(self.h, 1, *args))
        self._mode_axes = [a for a in range(3) if tables[a] is not None]

    def _modes_out(self, raw):
        """[..., 64 W, periodic axes, 2] doubles -> complex128 [..., S, 3], NaN on the open axes."""
        out = np.full(raw.shape[:-3] + (self.n_samples, 3), complex(np.nan, np.nan), dtype=np.complex128)
        for k, a in enumerate(self._mode_axes):  # the parts are stored as they are: no arithmetic that could turn -0.0 into 0.0
            out.real[..., a] = raw[..., :self.n_samples, k, 0]
            out.imag[..., a] = raw[..., :self.n_samples, k, 1]
        return out

    def modes(self):
        """complex128 (n_temps, S, 3): the k_min modes of the planes as they are, NaN on the open axes."""
        if not getattr(self, "_mode_axes", None):
            raise ValueError("msc_modes: call set_correlation first")
        raw = np.zeros((self.n_temps, self.words * 64, len(self._mode_axes), 2), np.float64)
        self.ctx.check(self.lib.tsu_msc_modes(self.h, _ptr(raw, _f64p)))
        return self._modes_out(raw)

    def pt_history_modes(self, n_rows):
        """complex128 (n_rows, n_temps, S, 3): the modes the last ``pt_run`` recorded."""
        if not getattr(self, "_mode_axes", None):
            raise ValueError("msc_pt_history_modes: call set_correlation first")
        raw = np.zeros((int(n_rows), self.n_temps, self.words * 64, len(self._mode_axes), 2), np.float64)
        self.ctx.check(self.lib.tsu_msc_pt_history_modes(self.h, int(n_rows), _ptr(raw, _f64p)))
        return self._modes_out(raw)

    # ---- real space and quenches (tsu_msc_c4 / _snapshot* / _quench_*): C_d[r] of the overlap field, two-time correlations
    def _c4_arrays(self, lead=()):
        cols = self.words * 64
        return [np.zeros(tuple(lead) + (self.n_temps, cols, n // 2 + 1), np.int64) if p else None for n, p in zip(self.shape, self.periodic)]

    def _c4_out(self, arrays):
        return tuple(None if x is None else x[..., :self.n_samples, :].copy() for x in arrays)

    def c4(self):
        """(C_z, C_r, C_c): int64 (n_temps, S, L_d / 2 + 1) sums of f_x f_{x + r e_d} per periodic axis, None for an open one; pad
        columns dropped."""
        out = self._c4_arrays()
        self.ctx.check(self.lib.tsu_msc_c4(self.h, *(None if x is None else _ptr(x, _i64p) for x in out)))
        return self._c4_out(out)

    def snapshot_slots(self, n):
        self.ctx.check(self.lib.tsu_msc_snapshot_slots(self.h, int(n)))

    def snapshot(self, slot=0):
        self.ctx.check(self.lib.tsu_msc_snapshot(self.h, int(slot)))

    def snapshot_overlap(self, slot=0):
        """int64 (n_temps, replicas, S): sum_x s_x(now) s_x(snapshot) per plane and sample; pad columns dropped."""
        out = np.zeros((self.n_temps, self.replicas, self.words * 64), np.int64)
        self.ctx.check(self.lib.tsu_msc_snapshot_overlap(self.h, int(slot), _ptr(out, _i64p)))
        return out[..., :self.n_samples].copy()

    def quench_run(self, times, sweep0=0, wait_index=()):
        t = np.ascontiguousarray(times, dtype=np.int32).ravel()
        wi = np.ascontiguousarray(wait_index, dtype=np.int32).ravel()
        self.ctx.check(self.lib.tsu_msc_quench_run(self.h, t.size, _ptr(t, _i32p), _counter("sweep0", sweep0), wi.size,
                                                   _ptr(wi, _i32p) if wi.size else None))
        self._quench_shape = (int(t.size), int(wi.size))

    def quench_history(self):
        """The rows of the last ``quench_run``: (unsat, sum, q, q_link) as :meth:`pt_history` gives them, the 3-tuple of
        :meth:`c4` with a leading time axis, and two_time int64 (n_wait, n_times, n_temps, replicas, S)."""
        n, nw = self._quench_shape
        cols, S = self.words * 64, self.n_samples
        unsat = np.zeros((n, self.n_temps, self.replicas, cols), np.int64)
        ssum = np.zeros_like(unsat)
        two = self.replicas == 2
        q = np.zeros((n, self.n_temps, cols), np.int64) if two else None
        ql = np.zeros((n, self.n_temps, cols), np.int64) if two else None
        c4 = self._c4_arrays((n,))
        tt = np.zeros((nw, n, self.n_temps, self.replicas, cols), np.int64)
        self.ctx.check(self.lib.tsu_msc_quench_history(
            self.h, n, _ptr(unsat, _i64p), _ptr(ssum, _i64p), _ptr(q, _i64p) if two else None, _ptr(ql, _i64p) if two else None,
            *(None if x is None else _ptr(x, _i64p) for x in c4), _ptr(tt, _i64p) if nw else None))
        meas = (unsat[..., :S].copy(), ssum[..., :S].copy(), q[..., :S].copy() if two else None, ql[..., :S].copy() if two else None)
        return meas, self._c4_out(c4), tt[..., :S].copy()


class _TemperingHandle:
    """What the tsu_pt2d and tsu_pt3d handles share: every call but create, set_disorder and the 2-D cluster moves.  A subclass
    sets ``_prefix`` (the C symbols' prefix) and, in its constructor, ``shape``, ``n_temps`` and ``n_ladders``, then calls
    ``_create`` with the shape arguments of its create function."""

    _prefix = None

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def _create(self, *shape_args):
        self._recorded = 0
        self._correlation = self._modes_recorded = False
        self._link = self._link_recorded = False
        h = _vp()
        self.ctx.check(self._fn("create")(self.ctx.h, *shape_args, self.n_temps, self.n_ladders, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def _set_disorder(self, arrays, h):
        a = [np.ascontiguousarray(x, dtype=np.float32).reshape(self.shape) for x in arrays]
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(self.shape)
        self.ctx.check(self._fn("set_disorder")(self.h, *[_ptr(x, _f32p) for x in a], None if hh is None else _ptr(hh, _f32p)))

    def set_temperatures(self, T):
        t = np.ascontiguousarray(T, dtype=np.float64).ravel()
        if t.size != self.n_temps:
            raise ValueError(f"need {self.n_temps} temperatures, got {t.size}")
        self.ctx.check(self._fn("set_temperatures")(self.h, _ptr(t, _f64p)))

    def init(self, seed, initial=0):
        """initial 0: random (the lattice's randomize(seed + walker index)); +1 / -1: all up / down."""
        self.ctx.check(self._fn("init")(self.h, _seed(seed), int(initial)))
        self._recorded = 0

    def run(self, n_rounds, swap_interval, swap=True, record=True):
        self.ctx.check(self._fn("run")(self.h, int(n_rounds), int(swap_interval), int(bool(swap)), int(bool(record))))
        self._recorded = int(n_rounds) if record else 0
        self._modes_recorded = bool(record) and self._correlation
        self._link_recorded = bool(record) and self._link

    def _periodic_flags(self):
        p = self.periodic
        return (bool(p),) * len(self.shape) if isinstance(p, (bool, np.bool_)) else tuple(bool(x) for x in p)

    def set_correlation(self, enable, tables=None):
        """Record the k_min modes of the periodic axes in every recording round.  ``tables``: per axis ``(cos, sin)`` float64 arrays of
        the axis's length made on the host, or None for an open axis."""
        n_axes = len(self.shape)
        tables = list(tables) if tables is not None else [None] * n_axes
        if len(tables) != n_axes:
            raise ValueError(f"need one table pair (or None) per axis, {n_axes} in all")
        keep, args = [], []
        for n, t in zip(self.shape, tables):
            if t is None:
                args += [None, None]
                continue
            pair = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in t]
            if len(pair) != 2 or pair[0].size != n or pair[1].size != n:
                raise ValueError(f"a table pair must be (cos, sin) of the axis's length {n}")
            keep += pair
            args += [_ptr(a, _f64p) for a in pair]
        self.ctx.check(self._fn("set_correlation")(self.h, int(bool(enable)), *args))
        if enable and not self._correlation:
            self._recorded = 0  # switching it on drops the previous run's rows
        self._correlation = bool(enable)

    def set_link_overlap(self, enable):
        """Record L, the link overlap of the two ladders' walkers at every slot, in every recording round (two ladders only)."""
        self.ctx.check(self._fn("set_link_overlap")(self.h, int(bool(enable))))
        if enable and not self._link:
            self._recorded = 0  # switching it on drops the previous run's rows
        self._link = bool(enable)

    def history_modes(self):
        """The last run's modes as complex128 (n_rounds, n_temps, n_periodic_axes); raises if that run recorded none."""
        n_per = sum(self._periodic_flags())
        n = self._recorded if self._modes_recorded else 0
        out = np.zeros((n, self.n_temps, n_per, 2))
        self.ctx.check(self._fn("history_modes")(self.h, _ptr(out, _f64p)))
        return out[..., 0] + 1j * out[..., 1]

    def profiles(self, slot):
        """Axis profiles (int64) of the walker now at ``slot``: of its spins, or with two ladders of the product of the two."""
        out = tuple(np.zeros(n, np.int64) for n in self.shape)
        self.ctx.check(self._fn("profiles")(self.h, int(slot), *[_ptr(a, _i64p) for a in out]))
        return out

    def history(self):
        """The last run's rows: E, M (sum of spins), walker as (n_rounds, n_ladders, n_temps); q as (n_rounds, n_temps) or None; q_link
        (n_rounds, n_temps), only if that run recorded the link overlap."""
        n, nl, R = self._recorded, self.n_ladders, self.n_temps
        E = np.zeros((n, nl, R))
        M = np.zeros((n, nl, R), np.int64)
        W = np.zeros((n, nl, R), np.int32)
        q = np.zeros((n, R), np.int64) if nl == 2 else None
        self.ctx.check(self._fn("history")(self.h, _ptr(E, _f64p), _ptr(M, _i64p), None if q is None else _ptr(q, _i64p),
                                           _ptr(W, _i32p)))
        out = {"E": E, "M": M, "walker": W, "q": q}
        if self._link_recorded:
            out["q_link"] = np.zeros((n, R), np.int64)
            self.ctx.check(self._fn("history_link")(self.h, _ptr(out["q_link"], _i64p)))
        return out

    def stats(self):
        nl, R = self.n_ladders, self.n_temps
        att, acc = np.zeros((nl, R - 1), np.int64), np.zeros((nl, R - 1), np.int64)
        trips, was = np.zeros((nl, R), np.int64), np.zeros((nl, R), np.int32)
        sw, rd = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self._fn("stats")(self.h, _ptr(att, _i64p), _ptr(acc, _i64p), _ptr(trips, _i64p), _ptr(was, _i32p),
                                         C.byref(sw), C.byref(rd)))
        return {"attempts": att, "accepts": acc, "round_trips": trips, "walker_at_slot": was, "sweep_count": sw.value,
                "round_count": rd.value}

    def energies(self):
        """(E, sum of spins) of every walker now, as (n_ladders, n_temps) arrays indexed by walker."""
        E = np.zeros((self.n_ladders, self.n_temps))
        M = np.zeros((self.n_ladders, self.n_temps), np.int64)
        self.ctx.check(self._fn("energies")(self.h, _ptr(E, _f64p), _ptr(M, _i64p)))
        return E, M

    def get_spins(self, ladder, slot):
        out = np.empty(self.shape, dtype=np.int8)
        self.ctx.check(self._fn("get_spins")(self.h, int(ladder), int(slot), _ptr(out, _i8p)))
        return out

    def set_spins(self, ladder, slot, spins):
        s = np.ascontiguousarray(spins, dtype=np.int8).reshape(self.shape)
        self.ctx.check(self._fn("set_spins")(self.h, int(ladder), int(slot), _ptr(s, _i8p)))

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self._fn("launch_count")(self.h, C.byref(n)))
        return n.value


class TemperingLattice(_TemperingHandle):
    """tsu_pt2d handle (K7 parallel tempering): n_ladders ladders of n_temps walkers of one rows x cols lattice sharing one
    disorder.  Walker w of ladder k has Philox key seed + k n_temps + w and starts at slot w."""

    _prefix = "tsu_pt2d_"

    def __init__(self, rows, cols, periodic, n_temps, n_ladders=1, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.rows, self.cols, self.periodic = int(rows), int(cols), bool(periodic)
        self.shape = (self.rows, self.cols)
        self.n_temps, self.n_ladders = int(n_temps), int(n_ladders)
        self._create(self.rows, self.cols, int(self.periodic))

    def set_disorder(self, J_right, J_down, h=None):
        self._set_disorder((J_right, J_down), h)

    def set_cluster_moves(self, every, t_max=float("inf")):
        """Replica cluster moves between the two ladders: a pass after the sweeps of every round t with t % every == 0 over the
        slots with T <= t_max; every = 0 switches them off."""
        self.ctx.check(self.lib.tsu_pt2d_set_cluster_moves(self.h, int(every), float(t_max)))

    def cluster_move(self):
        """One pass now (enqueued)."""
        self.ctx.check(self.lib.tsu_pt2d_cluster_move(self.h))

    def cluster_stats(self):
        R = self.n_temps
        passes, clusters, flipped = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
        m, nl = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self.lib.tsu_pt2d_cluster_stats(self.h, _ptr(passes, _i64p), _ptr(clusters, _i64p), _ptr(flipped, _i64p),
                                                       C.byref(m), C.byref(nl)))
        return {"passes": passes, "clusters": clusters, "flipped": flipped, "pass_count": m.value, "launches": nl.value}


class TemperingLattice3D(_TemperingHandle):
    """tsu_pt3d handle (K8 parallel tempering): n_ladders ladders of n_temps walkers of one depth x rows x cols lattice sharing one
    disorder.  Walker w of ladder k has Philox key seed + k n_temps + w and starts at slot w.  ``periodic``: a bool or a triple
    (p_z, p_r, p_c)."""

    _prefix = "tsu_pt3d_"

    def __init__(self, depth, rows, cols, periodic, n_temps, n_ladders=1, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.depth, self.rows, self.cols = int(depth), int(rows), int(cols)
        self.shape = (self.depth, self.rows, self.cols)
        self.periodic = periodic_axes(periodic)
        self.n_temps, self.n_ladders = int(n_temps), int(n_ladders)
        self._create(self.depth, self.rows, self.cols, sum(1 << a for a in range(3) if self.periodic[a]))

    def set_disorder(self, J_right, J_down, J_layer, h=None):
        self._set_disorder((J_right, J_down, J_layer), h)


ENSEMBLE_MAX_WALKERS = 65535


class _EnsembleHandle(_TemperingHandle):
    """What the tsu_pte2d and tsu_pte3d handles share: the ladders' calls with a leading sample axis on every array.  A subclass
    sets ``_prefix`` and, in its constructor, ``shape``, ``periodic``, ``n_samples``, ``n_temps`` and ``n_ladders``, then calls
    ``_create`` with the shape arguments of its create function."""

    def _create(self, *shape_args):
        self._recorded = 0
        self._correlation = self._modes_recorded = False
        self._link = self._link_recorded = False
        h = _vp()
        self.ctx.check(self._fn("create")(self.ctx.h, *shape_args, self.n_samples, self.n_temps, self.n_ladders, C.byref(h)))
        self.h = h

    def _set_disorder(self, arrays, h):
        full = (self.n_samples,) + tuple(self.shape)
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in arrays]
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.float32)
        for x in a + ([] if hh is None else [hh]):
            if x.shape != full:
                raise ValueError(f"disorder arrays must have shape {full}, got {x.shape}")
        self.ctx.check(self._fn("set_disorder")(self.h, *[_ptr(x, _f32p) for x in a], None if hh is None else _ptr(hh, _f32p)))

    def init(self, seeds, initial=0):
        """seeds: one uint64 per sample.  initial 0: random (walker (s, k, w) draws as the lattice's randomize(seeds[s] + k R + w));
        +1 / -1: all up / down."""
        sd = np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        if sd.shape != (self.n_samples,):
            raise ValueError(f"need {self.n_samples} seeds, got {sd.size}")
        self.ctx.check(self._fn("init")(self.h, _ptr(sd, _u64p), int(initial)))
        self._recorded = 0

    def history_modes(self):
        """The last run's modes as complex128 (n_rounds, n_samples, n_temps, n_periodic_axes); raises if that run recorded none."""
        n_per = sum(self._periodic_flags())
        n = self._recorded if self._modes_recorded else 0
        out = np.zeros((n, self.n_samples, self.n_temps, n_per, 2))
        self.ctx.check(self._fn("history_modes")(self.h, _ptr(out, _f64p)))
        return out[..., 0] + 1j * out[..., 1]

    def profiles(self, sample, slot):
        """Axis profiles (int64) of the walker of ``sample`` now at ``slot``: of its spins, or with two ladders of the product."""
        out = tuple(np.zeros(n, np.int64) for n in self.shape)
        self.ctx.check(self._fn("profiles")(self.h, int(sample), int(slot), *[_ptr(a, _i64p) for a in out]))
        return out

    def history(self):
        """The last run's rows: E, M (sum of spins), walker as (n_rounds, n_samples, n_ladders, n_temps); q as (n_rounds, n_samples,
        n_temps) or None; q_link like q, only if that run recorded the link overlap."""
        n, S, nl, R = self._recorded, self.n_samples, self.n_ladders, self.n_temps
        E = np.zeros((n, S, nl, R))
        M = np.zeros((n, S, nl, R), np.int64)
        W = np.zeros((n, S, nl, R), np.int32)
        q = np.zeros((n, S, R), np.int64) if nl == 2 else None
        self.ctx.check(self._fn("history")(self.h, _ptr(E, _f64p), _ptr(M, _i64p), None if q is None else _ptr(q, _i64p),
                                           _ptr(W, _i32p)))
        out = {"E": E, "M": M, "walker": W, "q": q}
        if self._link_recorded:
            out["q_link"] = np.zeros((n, S, R), np.int64)
            self.ctx.check(self._fn("history_link")(self.h, _ptr(out["q_link"], _i64p)))
        return out

    def stats(self):
        S, nl, R = self.n_samples, self.n_ladders, self.n_temps
        att, acc = np.zeros((S, nl, R - 1), np.int64), np.zeros((S, nl, R - 1), np.int64)
        trips, was = np.zeros((S, nl, R), np.int64), np.zeros((S, nl, R), np.int32)
        sw, rd = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self._fn("stats")(self.h, _ptr(att, _i64p), _ptr(acc, _i64p), _ptr(trips, _i64p), _ptr(was, _i32p),
                                         C.byref(sw), C.byref(rd)))
        return {"attempts": att, "accepts": acc, "round_trips": trips, "walker_at_slot": was, "sweep_count": sw.value,
                "round_count": rd.value}

    def energies(self):
        """(E, sum of spins) of every walker now, as (n_samples, n_ladders, n_temps) arrays indexed by walker."""
        E = np.zeros((self.n_samples, self.n_ladders, self.n_temps))
        M = np.zeros((self.n_samples, self.n_ladders, self.n_temps), np.int64)
        self.ctx.check(self._fn("energies")(self.h, _ptr(E, _f64p), _ptr(M, _i64p)))
        return E, M

    def get_spins(self, sample, ladder, slot):
        out = np.empty(self.shape, dtype=np.int8)
        self.ctx.check(self._fn("get_spins")(self.h, int(sample), int(ladder), int(slot), _ptr(out, _i8p)))
        return out

    def set_spins(self, sample, ladder, slot, spins):
        s = np.ascontiguousarray(spins, dtype=np.int8).reshape(self.shape)
        self.ctx.check(self._fn("set_spins")(self.h, int(sample), int(ladder), int(slot), _ptr(s, _i8p)))


class TemperingEnsemble(_EnsembleHandle):
    """tsu_pte2d handle (K7 tempering ensemble): n_samples disorder samples x n_ladders ladders x n_temps walkers of one rows x cols
    lattice, every pass of a round one launch for all samples.  Walker w of ladder k of sample s has Philox key
    seeds[s] + k n_temps + w and starts at slot w: sample s is a TemperingLattice on its disorder with seed seeds[s], bit for bit."""

    _prefix = "tsu_pte2d_"

    def __init__(self, rows, cols, periodic, n_samples, n_temps, n_ladders=1, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.rows, self.cols, self.periodic = int(rows), int(cols), bool(periodic)
        self.shape = (self.rows, self.cols)
        self.n_samples, self.n_temps, self.n_ladders = int(n_samples), int(n_temps), int(n_ladders)
        self._create(self.rows, self.cols, int(self.periodic))

    def set_disorder(self, J_right, J_down, h=None):
        """(n_samples, rows, cols) arrays, rounded once to fp32 (h=None: zero field)."""
        self._set_disorder((J_right, J_down), h)


class TemperingEnsemble3D(_EnsembleHandle):
    """tsu_pte3d handle (K8 tempering ensemble): TemperingEnsemble for depth x rows x cols lattices; sample s is a
    TemperingLattice3D on its disorder with seed seeds[s], bit for bit.  ``periodic``: a bool or a triple (p_z, p_r, p_c)."""

    _prefix = "tsu_pte3d_"

    def __init__(self, depth, rows, cols, periodic, n_samples, n_temps, n_ladders=1, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.depth, self.rows, self.cols = int(depth), int(rows), int(cols)
        self.shape = (self.depth, self.rows, self.cols)
        self.periodic = periodic_axes(periodic)
        self.n_samples, self.n_temps, self.n_ladders = int(n_samples), int(n_temps), int(n_ladders)
        self._create(self.depth, self.rows, self.cols, sum(1 << a for a in range(3) if self.periodic[a]))

    def set_disorder(self, J_right, J_down, J_layer, h=None):
        """(n_samples, depth, rows, cols) arrays, rounded once to fp32 (h=None: zero field)."""
        self._set_disorder((J_right, J_down, J_layer), h)


POPULATION_MAX = 65535


class _PopulationHandle:
    """What the tsu_pa2d and tsu_pa3d handles share: every call but create and set_disorder.  A subclass sets ``_prefix`` and, in
    its constructor, ``shape``, ``periodic`` and ``population``, then calls ``_create`` with the shape arguments of its create function."""

    _prefix = None

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def _create(self, *shape_args):
        self._recorded = None  # steps of the last run if it recorded
        self.n_steps = None    # steps of the schedule
        self.step_count = self.sweep_count = 0
        self._beta0 = 0.0
        self._resampled = False
        self._overlap = self._overlap_modes = False          # the switch
        self._overlap_recorded = self._modes_recorded = False  # what the last run recorded
        h = _vp()
        self.ctx.check(self._fn("create")(self.ctx.h, *shape_args, self.population, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def _set_disorder(self, arrays, h):
        a = [np.ascontiguousarray(x, dtype=np.float32).reshape(self.shape) for x in arrays]
        hh = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(self.shape)
        self.ctx.check(self._fn("set_disorder")(self.h, *[_ptr(x, _f32p) for x in a], None if hh is None else _ptr(hh, _f32p)))

    def set_schedule(self, betas):
        b = np.ascontiguousarray(betas, dtype=np.float64).ravel()
        self.ctx.check(self._fn("set_schedule")(self.h, _ptr(b, _f64p), int(b.size)))
        self.n_steps = int(b.size) - 1
        self._beta0 = float(b[0])

    def init(self, seed, initial_sweeps=0):
        """Walker i: key seed + i and the lattice's randomize(seed + i); initial_sweeps sweeps at 1 / beta[0] if beta[0] > 0."""
        self.ctx.check(self._fn("init")(self.h, _seed(seed), int(initial_sweeps)))
        self._recorded = None
        self.step_count = 0
        self.sweep_count = int(initial_sweeps) if self._beta0 > 0 else 0

    def run(self, n_steps, sweeps_per_step, resample=True, record=True):
        self.ctx.check(self._fn("run")(self.h, int(n_steps), int(sweeps_per_step), int(bool(resample)), int(bool(record))))
        self._recorded = int(n_steps) if record else None
        self._resampled = bool(resample)
        self._overlap_recorded = bool(record) and self._overlap
        self._modes_recorded = bool(record) and self._overlap_modes
        self.step_count += int(n_steps)
        self.sweep_count += int(n_steps) * int(sweeps_per_step)

    def history(self):
        """The last run's rows: E, M (n + 1, R), row 0 the population the run started from; W (uint32), parent (int32) (n, R);
        S, U (uint64), E_min (n,); resampled (n,) bool, whether that run resampled."""
        if self._recorded is None:
            raise ValueError("the last run recorded nothing")
        n, R = self._recorded, self.population
        out = {"E": np.zeros((n + 1, R)), "M": np.zeros((n + 1, R), np.int64), "W": np.zeros((n, R), np.uint32),
               "parent": np.zeros((n, R), np.int32), "S": np.zeros(n, np.uint64), "U": np.zeros(n, np.uint64), "E_min": np.zeros(n)}
        self.ctx.check(self._fn("history")(self.h, _ptr(out["E"], _f64p), _ptr(out["M"], _i64p), _ptr(out["W"], _u32p),
                                           _ptr(out["parent"], _i32p), _ptr(out["S"], _u64p), _ptr(out["U"], _u64p),
                                           _ptr(out["E_min"], _f64p)))
        out["resampled"] = np.full(n, self._resampled)
        if self._overlap_recorded:
            P = R // 2
            out["q"], out["q_link"] = np.zeros((n + 1, P), np.int64), np.zeros((n + 1, P), np.int64)
            modes = np.zeros((n + 1, P, sum(self._periodic_flags()), 2)) if self._modes_recorded else None
            self.ctx.check(self._fn("history_overlap")(self.h, _ptr(out["q"], _i64p), _ptr(out["q_link"], _i64p),
                                                       None if modes is None else _ptr(modes, _f64p)))
            if modes is not None:
                out["modes"] = modes[..., 0] + 1j * modes[..., 1]
        return out

    def _periodic_flags(self):
        p = self.periodic
        return (bool(p),) * len(self.shape) if isinstance(p, (bool, np.bool_)) else tuple(bool(x) for x in p)

    def set_overlap(self, enable, tables=None):
        """Record, in every recording run, q N and L of the walker pairs (i, i + population // 2) for the population the run starts
        from and after every step.  ``tables``: per axis ``(cos, sin)`` float64 arrays of the axis's length made on the host, or None
        for an open axis: then also the k_min modes of each pair's overlap field; ``tables=None``: q and L only."""
        n_axes = len(self.shape)
        with_modes = tables is not None
        tables = list(tables) if with_modes else [None] * n_axes
        if len(tables) != n_axes:
            raise ValueError(f"need one table pair (or None) per axis, {n_axes} in all")
        keep, args = [], []
        for n, t in zip(self.shape, tables):
            if t is None:
                args += [None, None]
                continue
            pair = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in t]
            if len(pair) != 2 or pair[0].size != n or pair[1].size != n:
                raise ValueError(f"a table pair must be (cos, sin) of the axis's length {n}")
            keep += pair
            args += [_ptr(a, _f64p) for a in pair]
        self.ctx.check(self._fn("set_overlap")(self.h, int(bool(enable)), *args))
        modes = bool(enable) and any(a is not None for a in args)
        if enable and (not self._overlap or modes != self._overlap_modes):
            self._recorded = None  # switching it on drops the previous run's rows
        self._overlap, self._overlap_modes = bool(enable), modes

    def energies(self):
        """(E, sum of spins) of every walker now, by walker."""
        E, M = np.zeros(self.population), np.zeros(self.population, np.int64)
        self.ctx.check(self._fn("energies")(self.h, _ptr(E, _f64p), _ptr(M, _i64p)))
        return E, M

    def get_spins(self, i):
        out = np.empty(self.shape, dtype=np.int8)
        self.ctx.check(self._fn("get_spins")(self.h, int(i), _ptr(out, _i8p)))
        return out

    def set_spins(self, i, spins):
        s = np.ascontiguousarray(spins, dtype=np.int8).reshape(self.shape)
        self.ctx.check(self._fn("set_spins")(self.h, int(i), _ptr(s, _i8p)))

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self._fn("launch_count")(self.h, C.byref(n)))
        return n.value


class PopulationLattice(_PopulationHandle):
    """tsu_pa2d handle (K7 population annealing): ``population`` walkers of one rows x cols lattice sharing one disorder.  Walker i
    has Philox key seed + i."""

    _prefix = "tsu_pa2d_"

    def __init__(self, rows, cols, periodic, population, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.rows, self.cols, self.periodic = int(rows), int(cols), bool(periodic)
        self.shape = (self.rows, self.cols)
        self.population = int(population)
        self._create(self.rows, self.cols, int(self.periodic))

    def set_disorder(self, J_right, J_down, h=None):
        self._set_disorder((J_right, J_down), h)


class PopulationLattice3D(_PopulationHandle):
    """tsu_pa3d handle (K8 population annealing): ``population`` walkers of one depth x rows x cols lattice sharing one disorder.
    ``periodic``: a bool or a triple (p_z, p_r, p_c)."""

    _prefix = "tsu_pa3d_"

    def __init__(self, depth, rows, cols, periodic, population, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.depth, self.rows, self.cols = int(depth), int(rows), int(cols)
        self.shape = (self.depth, self.rows, self.cols)
        self.periodic = periodic_axes(periodic)
        self.population = int(population)
        self._create(self.depth, self.rows, self.cols, sum(1 << a for a in range(3) if self.periodic[a]))

    def set_disorder(self, J_right, J_down, J_layer, h=None):
        self._set_disorder((J_right, J_down, J_layer), h)


def sweep_batch(lattices, n_sweeps, seeds, sweep0s, replicas=None):
    """n_sweeps sweeps of every lattice (own thresholds, seed, sweep counter, replica id); lattices that fit the
    one-workgroup kernel run concurrently in one launch.  Same results as sweeping them one by one."""
    n = len(lattices)
    if n == 0:
        return
    ctx = lattices[0].ctx
    hs = (_vp * n)(*[l.h for l in lattices])
    sd = (C.c_uint64 * n)(*_uint_array("seeds", seeds, np.uint64).tolist())
    s0 = (C.c_uint32 * n)(*_uint_array("sweep0s", sweep0s, np.uint32).tolist())
    rp = (C.c_uint32 * n)(*([0] * n if replicas is None else _uint_array("replicas", replicas, np.uint32, REPLICA_LIMIT).tolist()))
    ctx.check(lattices[0].lib.tsu_ising2d_sweep_batch(hs, n, int(n_sweeps), sd, s0, rp))


def cluster_sweep_batch(lattices, n_steps, Js, Ts, seeds, step0s, replicas=None):
    """n_steps Swendsen-Wang steps of every lattice (own J, T, seed, step counter, replica id); small lattices of one shape
    and boundary run in one launch.  Same results as stepping them one by one."""
    n = len(lattices)
    if n == 0:
        return
    ctx = lattices[0].ctx
    hs = (_vp * n)(*[l.h for l in lattices])
    js = (C.c_double * n)(*[float(v) for v in Js])
    ts = (C.c_double * n)(*[float(v) for v in Ts])
    sd = (C.c_uint64 * n)(*_uint_array("seeds", seeds, np.uint64).tolist())
    s0 = (C.c_uint32 * n)(*_uint_array("step0s", step0s, np.uint32).tolist())
    rp = (C.c_uint32 * n)(*([0] * n if replicas is None else _uint_array("replicas", replicas, np.uint32, REPLICA_LIMIT).tolist()))
    ctx.check(lattices[0].lib.tsu_ising2d_cluster_sweep_batch(hs, n, int(n_steps), js, ts, sd, s0, rp))


def _cluster_batch_3d(entry, lattices, n_steps, Ts, seeds, step0s, replicas):
    n = len(lattices)
    if n == 0:
        return
    ctx = lattices[0].ctx
    hs = (_vp * n)(*[l.h for l in lattices])
    ts = (C.c_double * n)(*[float(v) for v in Ts])
    sd = (C.c_uint64 * n)(*_uint_array("seeds", seeds, np.uint64).tolist())
    s0 = (C.c_uint32 * n)(*_uint_array("step0s", step0s, np.uint32).tolist())
    rp = (C.c_uint32 * n)(*([0] * n if replicas is None else _uint_array("replicas", replicas, np.uint32, REPLICA_LIMIT).tolist()))
    ctx.check(getattr(lattices[0].lib, entry)(hs, n, int(n_steps), ts, sd, s0, rp))


def cluster_sweep_batch_3d(lattices, n_steps, Ts, seeds, step0s, replicas=None):
    """n_steps Swendsen-Wang steps of every 3-D lattice (own disorder, T, seed, step counter, replica id); small lattices of one
    shape and boundary run in one launch.  Same results as stepping them one by one."""
    _cluster_batch_3d("tsu_ising3d_cluster_sweep_batch", lattices, n_steps, Ts, seeds, step0s, replicas)


def cluster_sweep_field_batch_3d(lattices, n_steps, Ts, seeds, step0s, replicas=None):
    """:func:`cluster_sweep_batch_3d` with ghost-spin steps (``Lattice3D.cluster_sweep_field``): every lattice's stored field takes
    part."""
    _cluster_batch_3d("tsu_ising3d_cluster_sweep_field_batch", lattices, n_steps, Ts, seeds, step0s, replicas)


def observables_batch(lattices):
    """[(sum of spins, sum over bonds)] of every lattice with one synchronisation."""
    n = len(lattices)
    if n == 0:
        return []
    hs = (_vp * n)(*[l.h for l in lattices])
    a, b = (C.c_int64 * n)(), (C.c_int64 * n)()
    lattices[0].ctx.check(lattices[0].lib.tsu_ising2d_observables_batch(hs, n, a, b))
    return [(int(a[i]), int(b[i])) for i in range(n)]


class DenseSystem:
    """tsu_dense handle: dense coupling matrix + bias resident on the GPU, {0,1} int8 state."""

    def __init__(self, J, bias=None, dtype=DTYPE_F64, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        J = np.asarray(J)
        if J.ndim != 2 or J.shape[0] != J.shape[1]:
            raise ValueError("Coupling matrix must be square")
        self.n = J.shape[0]
        Jc = np.ascontiguousarray(J, dtype=np.float64 if dtype == DTYPE_F64 else np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
        if b is not None and b.size != self.n:
            raise ValueError(f"bias must have length {self.n}")
        h = _vp()
        self.ctx.check(self.lib.tsu_dense_create(self.ctx.h, self.n, Jc.ctypes.data_as(_vp), int(dtype),
                                                 None if b is None else _ptr(b, _f64p), C.byref(h)))
        self.h = h
        # host mirror of the resident state, valid right after set_state / get_state: a caller that hands back the state it was
        # just given (the functional gibbs_sweep(state, ...) -> state idiom, compute_energy of that state) does not upload it again --
        # and the library keeps the fields J s + b it holds for exactly that state (tsu_dense_set_state would drop them)
        self._mirror = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_dense_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():  # at interpreter exit the process teardown frees the device memory
            self.close()

    def set_state(self, bits):
        b = np.ascontiguousarray(bits, dtype=np.int8).reshape(self.n)
        if self._mirror is not None and np.array_equal(b, self._mirror):
            return  # the device already holds exactly this state
        self.ctx.check(self.lib.tsu_dense_set_state(self.h, _ptr(b, _i8p)))
        self._mirror = b.copy()

    def get_state(self):
        out = np.empty(self.n, dtype=np.int8)
        self.ctx.check(self.lib.tsu_dense_get_state(self.h, _ptr(out, _i8p)))
        self._mirror = out.copy()
        return out

    def sweep(self, T, n_sweeps, seed=0, sweep0=0, replica=0, order=None, replay_uniforms=None):
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int64).reshape(n_sweeps, self.n)
        u = None if replay_uniforms is None else np.ascontiguousarray(replay_uniforms, dtype=np.float64).reshape(
            n_sweeps, self.n)
        self._mirror = None
        self.ctx.check(self.lib.tsu_dense_sweep(self.h, float(T), int(n_sweeps), None if o is None else _ptr(o, _i64p),
                                                _seed(seed), _counter("sweep0", sweep0), _replica(replica),
                                                None if u is None else _ptr(u, _f64p)))

    def sample(self, T, n_burnin, n_sweeps, n_samples, seed=0, sweep0=0, replica=0, order=None, replay_uniforms=None):
        """The whole sample_boltzmann run from the resident state in one C call: (n_samples, n) int8 of 0/1."""
        total = int(n_burnin) + int(n_samples) * int(n_sweeps)
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int64).reshape(total, self.n)
        u = None if replay_uniforms is None else np.ascontiguousarray(replay_uniforms, dtype=np.float64).reshape(total, self.n)
        out = np.empty((int(n_samples), self.n), dtype=np.int8)
        self._mirror = None
        self.ctx.check(self.lib.tsu_dense_sample(self.h, float(T), int(n_burnin), int(n_sweeps), int(n_samples),
                                                 None if o is None else _ptr(o, _i64p), _seed(seed), _counter("sweep0", sweep0), _replica(replica),
                                                 None if u is None else _ptr(u, _f64p), _ptr(out, _i8p)))
        return out

    def anneal(self, temperatures, seed=0, sweep0=0, replica=0, order=None, replay_uniforms=None):
        """One sweep per entry of ``temperatures`` from the resident state, every state recorded: (n_steps, n) int8."""
        t = np.ascontiguousarray(temperatures, dtype=np.float64)
        steps = t.size
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int64).reshape(steps, self.n)
        u = None if replay_uniforms is None else np.ascontiguousarray(replay_uniforms, dtype=np.float64).reshape(steps, self.n)
        out = np.empty((steps, self.n), dtype=np.int8)
        self._mirror = None
        self.ctx.check(self.lib.tsu_dense_anneal(self.h, _ptr(t, _f64p), steps, None if o is None else _ptr(o, _i64p), _seed(seed),
                                                 _counter("sweep0", sweep0), _replica(replica), None if u is None else _ptr(u, _f64p), _ptr(out, _i8p)))
        return out

    def sweep_replicas(self, states, temperatures, n_sweeps, seeds, sweep0s, replicas=None, replay_uniforms=None):
        """n_sweeps sweeps of every replica state (rows of ``states``) at its own temperature: (R, n) int8 of 0/1."""
        st = np.ascontiguousarray(states, dtype=np.int8).reshape(-1, self.n).copy()
        R = st.shape[0]
        t = np.ascontiguousarray(temperatures, dtype=np.float64).reshape(R)
        sd = _uint_array("seeds", seeds, np.uint64).reshape(R)
        s0 = _uint_array("sweep0s", sweep0s, np.uint32).reshape(R)
        rp = np.zeros(R, dtype=np.uint32) if replicas is None else _uint_array("replicas", replicas, np.uint32, REPLICA_LIMIT).reshape(R)
        u = None if replay_uniforms is None else np.ascontiguousarray(replay_uniforms, dtype=np.float64).reshape(R, int(n_sweeps), self.n)
        self._mirror = None  # (systems beyond the one-workgroup kernels are swept replica by replica through the resident state)
        self.ctx.check(self.lib.tsu_dense_sweep_replicas(self.h, R, _ptr(t, _f64p), int(n_sweeps), _ptr(st, _i8p), _ptr(sd, _u64p),
                                                         _ptr(s0, _u32p), _ptr(rp, _u32p), None if u is None else _ptr(u, _f64p)))
        return st

    def energy(self):
        e = C.c_double(0)
        self.ctx.check(self.lib.tsu_dense_energy(self.h, C.byref(e)))
        return e.value

    def launch_counts(self):
        """(launches of the owner-computes kernel k2_own, launches of the pipeline k2_pipe) made by this system so far."""
        c = (C.c_uint64 * 2)()
        self.ctx.check(self.lib.tsu_dense_launch_counts(self.h, c))
        return int(c[0]), int(c[1])

    def energies(self, states):
        """Energies of the given states ((k, n) of 0/1), evaluated on the device in one call; the resident state stays as it is."""
        st = np.ascontiguousarray(states, dtype=np.int8).reshape(-1, self.n)
        out = np.empty(st.shape[0], dtype=np.float64)
        if st.shape[0]:
            self.ctx.check(self.lib.tsu_dense_energies(self.h, _ptr(st, _i8p), int(st.shape[0]), _ptr(out, _f64p)))
        return out


def comm_unique_id() -> bytes:
    """128 opaque bytes that identify a new RCCL communicator: create on one rank, hand to the others."""
    lib = load_library()
    buf = np.zeros(128, dtype=np.uint8)
    rc = lib.tsu_comm_unique_id(_ptr(buf, _u8p))
    if rc != TSU_OK:
        raise HipError(f"tsu_comm_unique_id failed ({rc}): {lib.tsu_last_error(None).decode()}")
    return buf.tobytes()


class Comm:
    """tsu_comm handle: an RCCL communicator below the C ABI (one rank = one process = one GPU)."""

    def __init__(self, nranks, rank, unique_id: bytes, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.nranks, self.rank = int(nranks), int(rank)
        uid = np.frombuffer(unique_id, dtype=np.uint8).copy()
        if uid.size != 128:
            raise ValueError("the unique id is 128 bytes")
        h = _vp()
        self.ctx.check(self.lib.tsu_comm_create(self.ctx.h, self.nranks, self.rank, _ptr(uid, _u8p), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_comm_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def halo_exchange(self, lattice: "Lattice"):
        self.ctx.check(self.lib.tsu_ising2d_halo_exchange(lattice.h, self.h))

    def wait(self, timeout_s=120.0):
        """Bounded wait for the stream's sweeps and exchanges; returns the number of halo exchanges issued so far."""
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_comm_wait(self.h, float(timeout_s), C.byref(n)))
        return int(n.value)

    def allreduce(self, values):
        v = np.ascontiguousarray(values, dtype=np.int64).copy()
        self.ctx.check(self.lib.tsu_comm_allreduce_i64(self.h, _ptr(v, _i64p), v.size))
        return v


SPARSE_PLAN_FIELDS = ("route", "deg", "lo", "hi", "site_stride", "pair", "other", "v4", "o_lo", "o_n")
ROUTE_COLOR, ROUTE_STENCIL, ROUTE_SMALL = 0, 1, 2


def _plan_dicts(rec):
    return [dict(zip(SPARSE_PLAN_FIELDS, (int(v) for v in row))) for row in rec.reshape(-1, len(SPARSE_PLAN_FIELDS))]


def sparse_classify(row_ptr, col_idx, values, bias, color_offsets, order):
    """Host helper of the library (no GPU needed): the plan SparseSystem would get for this graph and colouring -- one dict per
    colour class with the fields SPARSE_PLAN_FIELDS (route: ROUTE_COLOR / ROUTE_STENCIL / ROUTE_SMALL; include/tsu_hip.h)."""
    lib = load_library()
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col_idx, dtype=np.int32)
    va = np.ascontiguousarray(values, dtype=np.float64)
    n = rp.size - 1
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64).reshape(n)
    co = np.ascontiguousarray(color_offsets, dtype=np.int32)
    od = np.ascontiguousarray(order, dtype=np.int32).reshape(n)
    rec = np.zeros((co.size - 1, len(SPARSE_PLAN_FIELDS)), dtype=np.int32)
    rc = lib.tsu_sparse_classify(n, _ptr(rp, _i64p), _ptr(ci, _i32p), _ptr(va, _f64p), None if b is None else _ptr(b, _f64p),
                                 co.size - 1, _ptr(co, _i32p), _ptr(od, _i32p), _ptr(rec, _i32p))
    if rc != TSU_OK:
        raise ValueError(lib.tsu_last_error(None).decode())
    return _plan_dicts(rec)


class SparseSystem:
    """tsu_sparse handle: a sparse coupling graph (CSR, bit couplings incl. an optional diagonal) with a proper colouring,
    swept one colour class at a time (K5).  ``order`` lists the sites colour by colour, ``color_offsets`` delimits the
    colours in it.  State is {0,1} int8 in site order."""

    def __init__(self, row_ptr, col_idx, values, bias, color_offsets, order, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        va = np.ascontiguousarray(values, dtype=np.float64)
        self.n = rp.size - 1
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64).reshape(self.n)
        co = np.ascontiguousarray(color_offsets, dtype=np.int32)
        od = np.ascontiguousarray(order, dtype=np.int32).reshape(self.n)
        self.n_colors = co.size - 1
        h = _vp()
        self.ctx.check(self.lib.tsu_sparse_create(self.ctx.h, self.n, _ptr(rp, _i64p), _ptr(ci, _i32p), _ptr(va, _f64p),
                                                  None if b is None else _ptr(b, _f64p), self.n_colors, _ptr(co, _i32p),
                                                  _ptr(od, _i32p), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_sparse_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def set_state(self, bits):
        b = np.ascontiguousarray(bits, dtype=np.int8).reshape(self.n)
        self.ctx.check(self.lib.tsu_sparse_set_state(self.h, _ptr(b, _i8p)))

    def get_state(self):
        out = np.empty(self.n, dtype=np.int8)
        self.ctx.check(self.lib.tsu_sparse_get_state(self.h, _ptr(out, _i8p)))
        return out

    def sweep(self, T, n_sweeps, seed=0, sweep0=0, replica=0):
        self.ctx.check(self.lib.tsu_sparse_sweep(self.h, float(T), int(n_sweeps), _seed(seed), _counter("sweep0", sweep0), _replica(replica)))

    def sample(self, T, n_burnin, n_sweeps, n_samples, seed=0, sweep0=0, replica=0):
        out = np.empty((int(n_samples), self.n), dtype=np.int8)
        self.ctx.check(self.lib.tsu_sparse_sample(self.h, float(T), int(n_burnin), int(n_sweeps), int(n_samples), _seed(seed),
                                                  _counter("sweep0", sweep0), _replica(replica), _ptr(out, _i8p)))
        return out

    def plan(self):
        """One dict per colour class (fields SPARSE_PLAN_FIELDS): the kernel the next sweep launches for it."""
        rec = np.zeros((self.n_colors, len(SPARSE_PLAN_FIELDS)), dtype=np.int32)
        for c in range(self.n_colors):
            self.ctx.check(self.lib.tsu_sparse_class_plan(self.h, c, _ptr(rec[c], _i32p)))
        return _plan_dicts(rec)

    def energy(self):
        """(-1/2 s'Js - b's of the resident bits, sum of the spins 2b-1)."""
        e, m = C.c_double(0), C.c_int64(0)
        self.ctx.check(self.lib.tsu_sparse_energy(self.h, C.byref(e), C.byref(m)))
        return e.value, m.value


SPARSE_BATCH_PLAN_FIELDS = ("route", "walkers_per_thread", "padded_walkers", "launches_per_sweep", "launches_per_round_fixed",
                            "energy_segments")
BATCH_ROUTE_COLOR, BATCH_ROUTE_SMALL = 0, 1
BATCH_MAX_TEMPS, BATCH_MAX_WALKERS = 256, 65535


class SparseBatch:
    """tsu_sparse_batch handle: ``n_ladders`` ladders of ``n_temps`` walkers on the graph of one :class:`SparseSystem` (which it keeps
    alive).  Walker g = ladder * n_temps + w starts at slot w; sweeps, energies and swap passes are batched launches and ``run`` waits
    for nothing (include/tsu_hip_sparse_batch.h).  States are {0,1} int8 in site order."""

    def __init__(self, graph, n_temps, n_ladders=1):
        self.graph = graph
        self.ctx, self.lib = graph.ctx, graph.lib
        self.n, self.R, self.nl = graph.n, int(n_temps), int(n_ladders)
        h = _vp()
        self.ctx.check(self.lib.tsu_sparse_batch_create(graph.h, self.R, self.nl, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_sparse_batch_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def set_temperatures(self, T):
        t = np.ascontiguousarray(T, dtype=np.float64).reshape(self.R)
        self.ctx.check(self.lib.tsu_sparse_batch_set_temperatures(self.h, _ptr(t, _f64p)))

    def init(self, seed, initial=0):
        self.ctx.check(self.lib.tsu_sparse_batch_init(self.h, _seed(seed), int(initial)))

    def set_state(self, ladder, slot, bits):
        b = np.ascontiguousarray(bits, dtype=np.int8).reshape(self.n)
        self.ctx.check(self.lib.tsu_sparse_batch_set_state(self.h, int(ladder), int(slot), _ptr(b, _i8p)))

    def get_state(self, ladder, slot):
        out = np.empty(self.n, dtype=np.int8)
        self.ctx.check(self.lib.tsu_sparse_batch_get_state(self.h, int(ladder), int(slot), _ptr(out, _i8p)))
        return out

    def run(self, n_rounds, swap_interval, do_swap=True, record=True):
        self.ctx.check(self.lib.tsu_sparse_batch_run(self.h, int(n_rounds), int(swap_interval), int(bool(do_swap)), int(bool(record))))
        if record:
            self._hist_rounds = int(n_rounds)
        else:
            self._hist_rounds = 0

    def history(self):
        """E, M, walker of the last recording run, each (rounds, n_ladders, n_temps)."""
        n = getattr(self, "_hist_rounds", 0)
        E = np.zeros((n, self.nl, self.R), dtype=np.float64)
        M = np.zeros((n, self.nl, self.R), dtype=np.int64)
        W = np.zeros((n, self.nl, self.R), dtype=np.int32)
        self.ctx.check(self.lib.tsu_sparse_batch_history(self.h, _ptr(E, _f64p), _ptr(M, _i64p), _ptr(W, _i32p)))
        return E, M, W

    def stats(self):
        att = np.zeros((self.nl, self.R - 1), dtype=np.int64)
        acc = np.zeros((self.nl, self.R - 1), dtype=np.int64)
        trips = np.zeros((self.nl, self.R), dtype=np.int64)
        was = np.zeros((self.nl, self.R), dtype=np.int32)
        sweeps = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_sparse_batch_stats(self.h, _ptr(att, _i64p), _ptr(acc, _i64p), _ptr(trips, _i64p), _ptr(was, _i32p),
                                                       C.byref(sweeps)))
        return {"attempts": att, "accepts": acc, "round_trips": trips, "walker_at_slot": was, "sweep_count": int(sweeps.value)}

    def energies(self):
        """(E, sum of spins) of every walker now, each (n_ladders, n_temps) indexed by WALKER."""
        E = np.zeros((self.nl, self.R), dtype=np.float64)
        M = np.zeros((self.nl, self.R), dtype=np.int64)
        self.ctx.check(self.lib.tsu_sparse_batch_energies(self.h, _ptr(E, _f64p), _ptr(M, _i64p)))
        return E, M

    def track_best(self, enable=True):
        self.ctx.check(self.lib.tsu_sparse_batch_track_best(self.h, int(bool(enable))))

    def best(self, ladder, bits=True):
        """(energy, bits or None, walker) of the ladder's lowest best energy (the first such walker)."""
        e, w = C.c_double(0), C.c_int32(0)
        out = np.empty(self.n, dtype=np.int8) if bits else None
        self.ctx.check(self.lib.tsu_sparse_batch_best(self.h, int(ladder), C.byref(e), None if out is None else _ptr(out, _i8p), C.byref(w)))
        return e.value, out, int(w.value)

    def plan(self):
        rec = np.zeros(len(SPARSE_BATCH_PLAN_FIELDS), dtype=np.int32)
        self.ctx.check(self.lib.tsu_sparse_batch_plan(self.h, _ptr(rec, _i32p)))
        return dict(zip(SPARSE_BATCH_PLAN_FIELDS, (int(v) for v in rec)))

    def launch_count(self):
        n = C.c_uint64(0)
        self.ctx.check(self.lib.tsu_sparse_batch_launch_count(self.h, C.byref(n)))
        return int(n.value)


class LangevinChains:
    """tsu_langevin handle: n_chains x dim float32 states with a separable quadratic, coupled quadratic or Gaussian-mixture energy."""

    def __init__(self, n_chains, dim, ctx=None):
        self.ctx = ctx or Context.default()
        self.lib = self.ctx.lib
        self.n_chains, self.dim = int(n_chains), int(dim)
        h = _vp()
        self.ctx.check(self.lib.tsu_langevin_create(self.ctx.h, self.n_chains, self.dim, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsu_langevin_destroy(self.h)
            self.h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():  # at interpreter exit the process teardown frees the device memory
            self.close()

    def set_state(self, x):
        xx = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float32), (self.n_chains, self.dim)))
        self.ctx.check(self.lib.tsu_langevin_set_state(self.h, _ptr(xx, _f32p)))

    def get_state(self):
        out = np.empty((self.n_chains, self.dim), dtype=np.float32)
        self.ctx.check(self.lib.tsu_langevin_get_state(self.h, _ptr(out, _f32p)))
        return out

    def set_energy(self, k, mu):
        kk = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float32), (self.dim,)))
        mm = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float32), (self.dim,)))
        self.ctx.check(self.lib.tsu_langevin_set_energy(self.h, _ptr(kk, _f32p), _ptr(mm, _f32p)))

    def set_coupling(self, A, b=None):
        """E = 1/2 x^T A x + b^T x with a symmetric (dim, dim) matrix: the steps that follow run the coupled kernel."""
        aa = np.ascontiguousarray(A, dtype=np.float32).reshape(self.dim, self.dim)
        bb = None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.float32), (self.dim,)))
        self.ctx.check(self.lib.tsu_langevin_set_coupling(self.h, _ptr(aa, _f32p), None if bb is None else _ptr(bb, _f32p)))

    def set_mixture(self, centers, weights, sigma=1.0, eps=1e-10):
        """E = -log(sum_i w_i exp(-||x - mu_i||^2 / (2 sigma_i^2)) + eps) (weights not renormalised): the steps that follow run the
        mixture kernels.  log w, 1/sigma^2 and log eps are formed in float64 and rounded to float32 once."""
        cc = np.asarray(centers, dtype=np.float64)
        if cc.ndim != 2 or cc.shape[1] != self.dim:
            raise ValueError(f"set_mixture: centers must have shape (K, {self.dim}), got {cc.shape}")
        K = cc.shape[0]
        w = np.broadcast_to(np.asarray(weights, dtype=np.float64), (K,))
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (K,))
        eps = float(eps)
        if not (np.all(np.isfinite(w)) and np.all(w > 0)):
            raise ValueError("set_mixture: weights must be finite and > 0")
        if not (np.all(np.isfinite(sg)) and np.all(sg > 0)):
            raise ValueError("set_mixture: sigma must be finite and > 0")
        if not (np.isfinite(eps) and eps >= 0):
            raise ValueError("set_mixture: eps must be finite and >= 0")
        c32 = np.ascontiguousarray(cc, dtype=np.float32)
        lw = np.ascontiguousarray(np.log(w), dtype=np.float32)
        iv = np.ascontiguousarray(1.0 / sg ** 2, dtype=np.float32)
        leps = float(np.float32(np.log(eps))) if eps > 0 else float("-inf")
        self.ctx.check(self.lib.tsu_langevin_set_mixture(self.h, int(K), _ptr(c32, _f32p), _ptr(lw, _f32p), _ptr(iv, _f32p), leps))

    def restart(self, x_init, amp, seed, chain0=0):
        xi = np.ascontiguousarray(np.broadcast_to(np.asarray(x_init, dtype=np.float32), (self.dim,)))
        self.ctx.check(self.lib.tsu_langevin_restart(self.h, _ptr(xi, _f32p), float(amp), _seed(seed), _counter("chain0", chain0)))

    def step(self, n_steps, dt, gamma, T, seed, step0=0, chain0=0, trajectory=False):
        traj = np.empty((n_steps, self.n_chains, self.dim), dtype=np.float32) if trajectory else None
        self.ctx.check(self.lib.tsu_langevin_step(self.h, int(n_steps), float(dt), float(gamma), float(T), _seed(seed),
                                                  _counter("step0", step0), _counter("chain0", chain0),
                                                  None if traj is None else _ptr(traj, _f32p)))
        return traj

    def set_kernel(self, steps_per_launch=0):
        self.ctx.check(self.lib.tsu_langevin_set_kernel(self.h, int(steps_per_launch)))
