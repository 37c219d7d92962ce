"""ctypes binding of include/wafer_hip.h.

`Context` mirrors the reference's private functions in src/grid.rs one to one
(evolve, compute_observables, get_norm_squared, normalise_wavefunction,
orthogonalise_wavefunction, solve) with device-resident state.  Host arrays are
numpy float64 in the reference's layout: C-order [x][y][z], shape (n + 2*ext).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WAFER_HIP_LIB: another build of the same library (same-box A/B runs of two kernel versions, tools/gpu_batch.sh ab_prev);
# it is still a HIP build of this engine -- there is no other implementation to point this at
_LIB = os.environ.get("WAFER_HIP_LIB") or os.path.join(_HERE, "libwafer_hip.so")

POTENTIALS = [
    "NoPotential", "Cube", "QuadWell", "Periodic", "Coulomb", "ComplexCoulomb",
    "ElipticalCoulomb", "SimpleCornell", "FullCornell", "Harmonic", "ComplexHarmonic",
    "Dodecahedron", "FromFile", "FromScript",
]  # config.rs:73-104
SYMMETRY = ["NotConstrained", "AboutZ", "AntisymAboutZ", "AboutY", "AntisymAboutY"]  # config.rs:184-197
INITIAL_CONDITIONS = ["FromFile", "Gaussian", "Coulomb", "Constant", "Boolean"]  # config.rs:151-170
CENTRAL_DIFFERENCE = {"ThreePoint": 1, "FivePoint": 2, "SevenPoint": 3}  # config.rs:224-238

WAFER_OK = 0
WAFER_ERR_INVALID = -1
WAFER_ERR_HIP = -2
WAFER_ERR_STATE = -4
WAFER_ERR_MAX_STEP = -5
RESAMPLE_PHI, RESAMPLE_POTENTIAL, RESAMPLE_POTSUB, RESAMPLE_STATE = 0, 1, 2, 3   # wafer_batch_resample's target / src_kind
RESAMPLE_BASIS = ("padded", "work")                                              # WAFER_BASIS_*
FLAG_SKIP_DT_CHECK = 1
FLAG_UNPLANNED_DIV = 2

EXPORTS = [
    "wafer_abi_version", "wafer_last_error", "wafer_ctx_create", "wafer_ctx_destroy",
    "wafer_synchronize", "wafer_set_potential_builtin", "wafer_set_potential_host",
    "wafer_download_array", "wafer_get_potsub", "wafer_set_initial_condition", "wafer_upload_phi",
    "wafer_download_phi", "wafer_upload_phi_resampled", "wafer_set_potential_resampled", "wafer_evolve", "wafer_observables", "wafer_norm2", "wafer_normalise",
    "wafer_orthogonalise", "wafer_push_state", "wafer_load_state", "wafer_download_state",
    "wafer_clone_state_to_phi", "wafer_num_states", "wafer_clear_states", "wafer_solve_state",
    "wafer_last_evolve_ms", "wafer_stencil_kernel_name", "wafer_stencil_kernel_instance", "wafer_stencil_steps_per_launch", "wafer_set_stencil_variant",
    "wafer_set_comm_hooks", "wafer_set_overlap", "wafer_set_stream", "wafer_get_slab_info",
    "wafer_get_device_info", "wafer_set_potsub", "wafer_set_potsub_resampled", "wafer_symmetrise", "wafer_download_phi_owned", "wafer_diag_div_check", "wafer_div_plan", "wafer_get_div_plan", "wafer_diag_div_planned", "wafer_div_plan_f32", "wafer_diag_div_planned_f32",
    "wafer_diag_copy_bw", "wafer_diag_checksum", "wafer_diag_download_window", "wafer_diag_dispatch", "wafer_set_halo_cycle", "wafer_diag_x2_passes",
    "wafer_peer_export", "wafer_peer_connect", "wafer_peer_disconnect",
    "wafer_batch_create", "wafer_batch_destroy", "wafer_batch_size", "wafer_batch_set_potential_builtin",
    "wafer_batch_set_potential_host", "wafer_batch_set_initial_condition", "wafer_batch_upload_phi", "wafer_batch_download_phi",
    "wafer_batch_evolve", "wafer_batch_observables", "wafer_batch_normalise", "wafer_batch_solve", "wafer_batch_last_evolve_ms",
    "wafer_batch_kernel_name", "wafer_batch_steps_per_launch", "wafer_batch_set_step_variant", "wafer_batch_diag_dispatch",
    "wafer_batch_diag_passes",
    "wafer_batch_load_state", "wafer_batch_download_state", "wafer_batch_push_state", "wafer_batch_num_states",
    "wafer_batch_clear_states", "wafer_batch_clone_state_to_phi", "wafer_batch_orthogonalise", "wafer_batch_norm2",
    "wafer_batch_evolve_state", "wafer_batch_solve_state",
    "wafer_batch_set_gs_variant", "wafer_batch_diag_gs", "wafer_batch_diag_gs_steps",
    "wafer_batch_create_mixed", "wafer_batch_create_mixed_states", "wafer_batch_num_shapes",
    "wafer_batch_symmetrise", "wafer_batch_set_potsub",
    "wafer_batch_resample", "wafer_batch_resample_member", "wafer_batch_last_resample_ms",
    "wafer_batch_set_potentials_builtin", "wafer_batch_set_initial_conditions", "wafer_batch_download_array", "wafer_batch_get_potsub",
    "wafer_batch_diag_member", "wafer_batch_diag_setup_counts",
    "wafer_ritz_solve", "wafer_ritz_matrices", "wafer_rotate_states", "wafer_ritz",
    "wafer_batch_ritz_matrices", "wafer_batch_rotate_states", "wafer_batch_ritz", "wafer_batch_diag_ritz_counts",
    "wafer_residuals", "wafer_residual_to_phi", "wafer_batch_residuals", "wafer_batch_diag_residual_counts",
    "wafer_evolve_states", "wafer_batch_evolve_states", "wafer_batch_diag_store_step", "wafer_batch_diag_store_counts",
    "wafer_filter_coefficients", "wafer_filter_states", "wafer_spectral_bound", "wafer_batch_filter_states", "wafer_batch_spectral_bound",
    "wafer_batch_diag_filter_counts",
    "wafer_moment_matrices", "wafer_batch_moment_matrices", "wafer_batch_diag_moment_counts",
]
RITZ_MAX = 8   # WAFER_RITZ_MAX
MOMENT_NAMES = ("s", "x", "y", "z", "r2")   # WAFER_MOMENT_S .. WAFER_MOMENT_R2
MOMENT_COUNT = len(MOMENT_NAMES)            # WAFER_MOMENT_COUNT


def moment_origin(nx: int, ny: int, nz: int) -> tuple:
    """the centres the moment matrices (and observables' r2) measure from, in 0-based work indices: (n + 1) / 2 per axis -- one cell
    above the geometric centre (n - 1) / 2, the reference's convention"""
    return ((nx + 1.) / 2., (ny + 1.) / 2., (nz + 1.) / 2.)
RESIDUAL_SOURCES = {"states": 0, "phi": 1}   # WAFER_RESIDUAL_STATES, WAFER_RESIDUAL_PHI


class _DivPlan(C.Structure):
    """wafer_div_plan_t (include/wafer_hip.h)"""
    _fields_ = [("den", C.c_double), ("zh", C.c_double), ("zl", C.c_double), ("checked", C.c_int32), ("n_candidates", C.c_int32),
                ("zl_shift", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class _DivPlanF32(C.Structure):
    """wafer_div_plan_f32_t (include/wafer_hip.h)"""
    _fields_ = [("den", C.c_float), ("zh", C.c_float), ("zl", C.c_float), ("checked", C.c_int32), ("zl_shift", C.c_int32)]


class WaferError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"wafer_hip error {code}: {msg}")
        self.code = code


class _PeerInfo(C.Structure):
    """wafer_peer_info (include/wafer_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("z_begin", C.c_uint32), ("z_count", C.c_uint32), ("halo_depth", C.c_uint32),
        ("pid", C.c_uint64), ("phi_addr", C.c_uint64 * 2), ("flags_addr", C.c_uint64), ("phi_alloc_offset", C.c_uint64 * 2),
        ("phi_ipc", (C.c_uint8 * 64) * 2), ("flags_ipc", C.c_uint8 * 64),
        ("process_nonce", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_uint32), ("device_uuid", C.c_uint8 * 16),
    ]


class _Params(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32),
        ("central_difference", C.c_int32), ("dtype", C.c_int32),
        ("dn", C.c_double), ("dt", C.c_double), ("mass", C.c_double), ("sig", C.c_double),
        ("max_states", C.c_uint32), ("device", C.c_int32),
        ("z_begin", C.c_uint32), ("z_count", C.c_uint32), ("halo_depth", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class _Obs(C.Structure):
    _fields_ = [("energy", C.c_double), ("norm2", C.c_double), ("v_infinity", C.c_double),
                ("r2", C.c_double)]


class _Record(C.Structure):
    _fields_ = [("step", C.c_uint64), ("tau", C.c_double), ("obs", _Obs), ("diff", C.c_double)]


class _ObsOut(C.Structure):
    _fields_ = [("state", C.c_uint32), ("energy", C.c_double), ("binding_energy", C.c_double),
                ("r", C.c_double), ("l_r", C.c_double)]


class _DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("arch", C.c_char * 64), ("compute_units", C.c_uint32),
                ("memory_clock_khz", C.c_uint32), ("memory_bus_bits", C.c_uint32), ("l2_bytes", C.c_uint32),
                ("total_bytes", C.c_uint64)]


class _SlabInfo(C.Structure):
    _fields_ = [("z_begin", C.c_uint32), ("z_count", C.c_uint32), ("halo_depth", C.c_uint32),
                ("ext", C.c_uint32), ("plane_elems", C.c_uint64), ("elem_bytes", C.c_uint64)]


HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_size_t, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

_lib = None


def library_path() -> str:
    return _LIB


def load_library():
    """Loads libwafer_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process.  PyTorch's ROCm wheels bundle their own libamdhip64.so.7 /
    # libhsa-runtime64 with the SAME sonames as /opt/rocm's, so whichever loads first serves
    # every later user.  If this library pulled in /opt/rocm's first, a later torch.cuda init
    # fails ("No HIP GPUs are available") and slab.py could not alias the engine's buffers and
    # streams.  Importing torch first makes its runtime the process-wide one.  A host without
    # torch (a Rust binary, WAFER_PRELOAD_TORCH=0) simply links /opt/rocm's.
    if os.environ.get("WAFER_PRELOAD_TORCH", "1") != "0":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(_LIB):
        raise ImportError(
            f"{_LIB} is missing: build it with `python -m wafer_amd.build` "
            "(hipcc --offload-arch=gfx950). The engine has no CPU fallback.")
    L = C.CDLL(_LIB)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.wafer_abi_version.restype = C.c_int
    L.wafer_last_error.restype = C.c_char_p
    L.wafer_ctx_create.argtypes = [C.POINTER(_Params), C.POINTER(vp)]
    L.wafer_ctx_destroy.argtypes = [vp]
    L.wafer_synchronize.argtypes = [vp]
    L.wafer_set_potential_builtin.argtypes = [vp, C.c_int]
    L.wafer_set_potential_host.argtypes = [vp, dp, C.c_int, C.c_double, dp]
    L.wafer_download_array.argtypes = [vp, C.c_int, dp]
    L.wafer_get_potsub.argtypes = [vp, C.POINTER(C.c_int), dp]
    L.wafer_set_potsub.argtypes = [vp, C.c_int, C.c_double, dp]
    L.wafer_set_potsub_resampled.argtypes = [vp, dp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.wafer_symmetrise.argtypes = [vp, C.c_int]
    L.wafer_download_phi_owned.argtypes = [vp, dp]
    L.wafer_diag_div_check.argtypes = [vp, C.c_double, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.wafer_div_plan.argtypes = [C.c_double, C.POINTER(_DivPlan), dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.wafer_get_div_plan.argtypes = [vp, C.POINTER(_DivPlan)]
    L.wafer_diag_div_planned.argtypes = [vp, C.POINTER(_DivPlan), C.c_uint64, C.c_uint64, C.c_int, C.c_int, dp, C.c_size_t,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.wafer_div_plan_f32.argtypes = [C.c_float, C.POINTER(_DivPlanF32)]
    L.wafer_diag_div_planned_f32.argtypes = [vp, C.POINTER(_DivPlanF32), C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.wafer_diag_copy_bw.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    L.wafer_diag_checksum.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.wafer_diag_x2_passes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.wafer_diag_dispatch.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.wafer_diag_download_window.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, dp]
    L.wafer_peer_export.argtypes = [vp, C.POINTER(_PeerInfo)]
    L.wafer_peer_connect.argtypes = [vp, C.POINTER(_PeerInfo), C.POINTER(_PeerInfo)]
    L.wafer_peer_disconnect.argtypes = [vp]
    L.wafer_set_initial_condition.argtypes = [vp, C.c_int, C.c_uint64]
    L.wafer_upload_phi.argtypes = [vp, dp]
    L.wafer_download_phi.argtypes = [vp, dp]
    u32p = C.POINTER(C.c_uint32)
    L.wafer_upload_phi_resampled.argtypes = [vp, dp, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    L.wafer_set_potential_resampled.argtypes = [vp, dp, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    L.wafer_evolve.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.wafer_observables.argtypes = [vp, C.POINTER(_Obs)]
    L.wafer_norm2.argtypes = [vp, dp]
    L.wafer_normalise.argtypes = [vp, C.c_double]
    L.wafer_orthogonalise.argtypes = [vp, C.c_uint32]
    L.wafer_push_state.argtypes = [vp]
    L.wafer_load_state.argtypes = [vp, C.c_uint32, dp]
    L.wafer_download_state.argtypes = [vp, C.c_uint32, dp]
    L.wafer_clone_state_to_phi.argtypes = [vp, C.c_uint32]
    L.wafer_num_states.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.wafer_clear_states.argtypes = [vp]
    L.wafer_ritz_solve.argtypes = [C.c_uint32, dp, dp, dp, dp]
    L.wafer_ritz_matrices.argtypes = [vp, C.c_uint32, dp, dp]
    L.wafer_rotate_states.argtypes = [vp, C.c_uint32, dp]
    L.wafer_ritz.argtypes = [vp, C.c_uint32, dp, dp, dp, dp]
    L.wafer_residuals.argtypes = [vp, C.c_int, C.c_uint32, dp, dp, dp, dp]
    L.wafer_residual_to_phi.argtypes = [vp, C.c_uint32, C.c_double]
    L.wafer_moment_matrices.argtypes = [vp, C.c_uint32, dp]
    L.wafer_solve_state.argtypes = [vp, C.c_uint32, C.c_double, C.c_uint64, C.c_int, C.c_uint64,
                                    C.POINTER(_Record), C.c_size_t, C.POINTER(C.c_size_t),
                                    C.POINTER(_ObsOut)]
    L.wafer_last_evolve_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    L.wafer_stencil_kernel_name.argtypes = [vp]
    L.wafer_stencil_kernel_name.restype = C.c_char_p
    L.wafer_stencil_kernel_instance.argtypes = [vp]
    L.wafer_stencil_kernel_instance.restype = C.c_char_p
    L.wafer_stencil_steps_per_launch.argtypes = [vp]
    L.wafer_set_stencil_variant.argtypes = [vp, C.c_int]
    L.wafer_set_comm_hooks.argtypes = [vp, HALO_FN, ALLREDUCE_FN, vp]
    L.wafer_set_overlap.argtypes = [vp, C.c_int]
    L.wafer_set_halo_cycle.argtypes = [vp, C.c_int]
    L.wafer_set_stream.argtypes = [vp, vp]
    L.wafer_get_slab_info.argtypes = [vp, C.POINTER(_SlabInfo)]
    L.wafer_get_device_info.argtypes = [vp, C.POINTER(_DeviceInfo)]
    u8p = C.POINTER(C.c_uint8)
    L.wafer_batch_create.argtypes = [C.POINTER(_Params), C.c_uint32, C.POINTER(vp)]
    L.wafer_batch_create_mixed.argtypes = [C.POINTER(_Params), C.c_uint32, C.POINTER(vp)]
    L.wafer_batch_create_mixed_states.argtypes = [C.POINTER(_Params), C.c_uint32, C.POINTER(vp)]
    L.wafer_batch_num_shapes.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.wafer_batch_destroy.argtypes = [vp]
    L.wafer_batch_size.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.wafer_batch_set_potential_builtin.argtypes = [vp, C.c_uint32, C.c_int]
    L.wafer_batch_set_potential_host.argtypes = [vp, C.c_uint32, dp, C.c_int, C.c_double, dp]
    L.wafer_batch_set_initial_condition.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint64]
    L.wafer_batch_upload_phi.argtypes = [vp, C.c_uint32, dp]
    L.wafer_batch_download_phi.argtypes = [vp, C.c_uint32, dp]
    L.wafer_batch_evolve.argtypes = [vp, u8p, C.c_uint64]
    L.wafer_batch_observables.argtypes = [vp, C.POINTER(_Obs)]
    L.wafer_batch_normalise.argtypes = [vp, u8p, dp]
    L.wafer_batch_solve.argtypes = [vp, C.c_double, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(_Record), C.c_size_t,
                                    C.POINTER(C.c_size_t), C.POINTER(_ObsOut), C.POINTER(C.c_int)]
    L.wafer_batch_last_evolve_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    L.wafer_batch_kernel_name.argtypes = [vp]
    L.wafer_batch_kernel_name.restype = C.c_char_p
    L.wafer_batch_steps_per_launch.argtypes = [vp]
    L.wafer_batch_set_step_variant.argtypes = [vp, C.c_int]
    L.wafer_batch_diag_dispatch.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.wafer_batch_diag_passes.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.wafer_batch_load_state.argtypes = [vp, C.c_uint32, C.c_uint32, dp]
    L.wafer_batch_download_state.argtypes = [vp, C.c_uint32, C.c_uint32, dp]
    L.wafer_batch_push_state.argtypes = [vp, u8p]
    L.wafer_batch_num_states.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.wafer_batch_clear_states.argtypes = [vp, u8p]
    L.wafer_batch_clone_state_to_phi.argtypes = [vp, u8p, C.c_uint32]
    L.wafer_batch_orthogonalise.argtypes = [vp, u8p, C.c_uint32]
    L.wafer_batch_norm2.argtypes = [vp, dp]
    L.wafer_batch_evolve_state.argtypes = [vp, u8p, C.c_uint32, C.c_uint64]
    L.wafer_batch_solve_state.argtypes = [vp, C.c_uint32, C.c_double, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(_Record), C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(_ObsOut), C.POINTER(C.c_int)]
    L.wafer_batch_set_gs_variant.argtypes = [vp, C.c_int]
    L.wafer_batch_diag_gs.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.wafer_batch_diag_gs_steps.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.wafer_batch_symmetrise.argtypes = [vp, u8p, C.POINTER(C.c_int)]
    L.wafer_batch_set_potsub.argtypes = [vp, C.c_uint32, C.c_int, C.c_double, dp]
    L.wafer_batch_resample.argtypes = [vp, u8p, C.c_int, C.c_uint32, dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.wafer_batch_resample_member.argtypes = [vp, u8p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int]
    L.wafer_batch_last_resample_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.wafer_batch_set_potentials_builtin.argtypes = [vp, u8p, C.POINTER(C.c_int)]
    L.wafer_batch_set_initial_conditions.argtypes = [vp, u8p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.wafer_batch_download_array.argtypes = [vp, C.c_uint32, C.c_int, dp]
    L.wafer_batch_get_potsub.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int), dp]
    L.wafer_batch_diag_member.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.wafer_batch_diag_setup_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    u32p = C.POINTER(C.c_uint32)
    L.wafer_batch_ritz_matrices.argtypes = [vp, u8p, u32p, dp, dp]
    L.wafer_batch_rotate_states.argtypes = [vp, u8p, u32p, dp]
    L.wafer_batch_ritz.argtypes = [vp, u8p, u32p, dp, dp, dp, dp, C.POINTER(C.c_int)]
    L.wafer_batch_diag_ritz_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.wafer_batch_residuals.argtypes = [vp, C.c_int, u8p, u32p, dp, dp, dp, dp, C.POINTER(C.c_int)]
    L.wafer_batch_diag_residual_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.wafer_batch_moment_matrices.argtypes = [vp, u8p, u32p, dp]
    L.wafer_batch_diag_moment_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.wafer_evolve_states.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.wafer_batch_evolve_states.argtypes = [vp, u8p, u32p, C.c_uint64]
    L.wafer_batch_diag_store_step.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.wafer_batch_diag_store_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.wafer_filter_coefficients.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_double, dp, dp, dp]
    L.wafer_filter_states.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double]
    L.wafer_spectral_bound.argtypes = [vp, dp]
    L.wafer_batch_filter_states.argtypes = [vp, u8p, u32p, C.c_uint32, dp, dp, dp]
    L.wafer_batch_spectral_bound.argtypes = [vp, u8p, dp]
    L.wafer_batch_diag_filter_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if L.wafer_abi_version() != 1:
        raise ImportError("libwafer_hip.so ABI version mismatch")
    _lib = L
    return L


@dataclass
class Params:
    """The subset of Config (config.rs:292-333) the hot path reads + engine knobs."""
    nx: int
    ny: int
    nz: int
    dn: float
    dt: float
    mass: float = 1.0
    sig: float = 1.0
    central_difference: int = 1      # 1/2/3 or "ThreePoint"/"FivePoint"/"SevenPoint"
    dtype: str = "f64"               # "f64" | "f32" (fp32 storage, fp64 arithmetic) | "f32fast" (+ fp32 step arithmetic)
    max_states: int = 4
    device: int = 0
    z_begin: int = 0
    z_count: int = 0                 # 0 = whole grid
    halo_depth: int = 0              # 0 = ext
    skip_dt_check: bool = False
    unplanned_div: bool = False      # WAFER_FLAG_UNPLANNED_DIV: x / (c dn^2 m) always with the extra Markstein round

    @property
    def ext(self) -> int:
        cd = self.central_difference
        return CENTRAL_DIFFERENCE[cd] if isinstance(cd, str) else int(cd)

    @property
    def padded_shape(self):
        e = self.ext
        return (self.nx + 2 * e, self.ny + 2 * e, self.nz + 2 * e)

    @property
    def work_shape(self):
        return (self.nx, self.ny, self.nz)

    def c(self) -> _Params:
        return _Params(C.sizeof(_Params), self.nx, self.ny, self.nz, self.ext,
                       {"f64": 0, "f32": 1, "f32fast": 2}[self.dtype], self.dn, self.dt, self.mass, self.sig,
                       self.max_states, self.device, self.z_begin, self.z_count, self.halo_depth,
                       (FLAG_SKIP_DT_CHECK if self.skip_dt_check else 0) | (FLAG_UNPLANNED_DIV if self.unplanned_div else 0))


def div_plan(den: float, max_candidates: int = 4096):
    """(plan, candidates): wafer_div_plan -- host only, no GPU: how the step kernels will divide by `den`, and the significands
    (doubles in [2^52, 2^53)) the plan had to try"""
    L = load_library()
    p = _DivPlan()
    cand = np.zeros(max_candidates)
    n = C.c_size_t(0)
    rc = L.wafer_div_plan(den, C.byref(p), _dp(cand), cand.size, C.byref(n))
    if rc != 0:
        raise WaferError(rc, L.wafer_last_error().decode())
    return p, cand[:n.value].copy()


def div_plan_f32(den: float) -> _DivPlanF32:
    """wafer_div_plan_f32 -- host only: the fp32 plan of x / den (all 2^23 significands tried)"""
    L = load_library()
    p = _DivPlanF32()
    rc = L.wafer_div_plan_f32(den, C.byref(p))
    if rc != 0:
        raise WaferError(rc, L.wafer_last_error().decode())
    return p


def ritz_solve(h, s):
    """(evals, coef): wafer_ritz_solve -- host only, no GPU: the Rayleigh-Ritz step of the (k, k) matrices h and s, k <= RITZ_MAX.
    evals ascend; coef[j, a] is the component of input state j in output state a"""
    L = load_library()
    h = np.ascontiguousarray(h, dtype=np.float64)
    s = np.ascontiguousarray(s, dtype=np.float64)
    if h.ndim != 2 or h.shape[0] != h.shape[1] or s.shape != h.shape:
        raise ValueError(f"h and s must be square matrices of one size, not {h.shape} and {s.shape}")
    k = h.shape[0]
    evals, coef = np.zeros(max(k, 1)), np.zeros((max(k, 1), max(k, 1)))
    rc = L.wafer_ritz_solve(k, _dp(h), _dp(s), _dp(evals), _dp(coef))
    if rc != 0:
        raise WaferError(rc, L.wafer_last_error().decode())
    return evals, coef


def _dp(a: np.ndarray):
    if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("host arrays must be C-contiguous float64")
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _enum_entries(names, table, n_members: int, mask, what: str) -> list:
    """names (one per member: a name of `table` or its index) as the ints the library takes.  The entries of members that `mask`
    (None: everyone listed) leaves out are not looked at: an int goes through, anything else becomes 0.  A listed name the table does not hold is a ValueError; an
    int goes through as it is (the library checks it)."""
    names = list(names)
    if len(names) != n_members:
        raise ValueError("%s names must hold one entry per member (%d given, the batch has %d)" % (what, len(names), n_members))
    out = []
    for m, name in enumerate(names):
        if mask is not None and not mask[m]:
            out.append(name if isinstance(name, int) and not isinstance(name, bool) else 0)
        elif isinstance(name, str):
            if name not in table:
                raise ValueError("member %d: unknown %s %r" % (m, what, name))
            out.append(table.index(name))
        else:
            out.append(int(name))
    return out


# ---- subspace iteration on the state stores: the driver, written once -----------------------------------------------------------
BLOCK_CONVERGED, BLOCK_MAX_BLOCKS, BLOCK_DEPENDENT = WAFER_OK, WAFER_ERR_MAX_STEP, WAFER_ERR_STATE


def _solve_loop(ks, tolerance, per_block, max_blocks, advance, ritz, residuals, worst, dependent, exhausted, first=None) -> list:
    """What block_solve_loop and filtered_solve_loop share (their statuses are the same three codes): the result dicts, the Ritz step
    with its linearly-dependent branch, the residual call, the row record, the members that leave `going`, the max_blocks message.
        advance(going, block, out)  moves the states of the members in `going` on by one block -> those it moved (the others got their
                                    status and message from it and are done)
        worst(o, m)                 the number that decides for member m: it is done when this is < tolerance
        dependent, exhausted        the two messages: % (m, block, steps, k, per_block) and % (m, max_blocks, worst, tolerance)
        first(going)                where given and anyone takes part: called once, and one Ritz step on the starts (block 0) follows"""
    out = [None if n == 0 else dict(status=BLOCK_MAX_BLOCKS, message="", blocks=0, steps=0, evals=None, diff=None, rho=None, rows=[])
           for n in ks]
    going = [m for m, n in enumerate(ks) if n > 0]

    def solve(members, block):
        """Ritz on `members`: evals and diff into out, -> those it succeeded on"""
        solved = ritz(list(members))
        alive = []
        for m in members:
            status, evals = solved[m]
            o = out[m]
            if status != WAFER_OK:
                o["status"] = BLOCK_DEPENDENT
                o["message"] = dependent % (m, block, o["steps"], ks[m], per_block)
                continue
            evals = np.array(evals, dtype=np.float64)[:ks[m]]
            o["diff"] = np.full(ks[m], np.inf) if o["evals"] is None else np.abs(evals - o["evals"])
            o["evals"] = evals
            alive.append(m)
        return alive

    if first is not None and going:
        first(list(going))
        going = solve(going, 0)
    for block in range(1, max_blocks + 1):
        going = advance(going, block, out) if going else []
        if not going:
            break
        for m in going:
            out[m]["blocks"], out[m]["steps"] = block, block * per_block
        alive = solve(going, block)
        rho = residuals(list(alive), {m: out[m]["evals"] for m in alive}) if alive else {}
        going = []
        for m in alive:
            o = out[m]
            o["rho"] = np.array(rho[m], dtype=np.float64)[:ks[m]]
            o["rows"].append(dict(block=block, steps=o["steps"], evals=o["evals"].copy(), diff=o["diff"].copy(), rho=o["rho"].copy()))
            if worst(o, m) < tolerance:
                o["status"] = BLOCK_CONVERGED
            else:
                going.append(m)
    for m in going:
        out[m]["message"] = exhausted % (m, max_blocks, worst(out[m], m), tolerance)
    return out


def block_solve_loop(step, ritz, residuals, k, tolerance: float, steps_per_block: int, max_blocks: int) -> list:
    """Subspace iteration over a set of members, backend-free (Context.solve_block, Batch.solve_block and the numpy model of the
    tests all call this).  k: one state count per member (0 or None: the member takes no part).  Three callables over the members
    still `going` (a sorted list of member indices):
        step(going, n)              advances the first k[m] stored states of every member in `going` by n plain steps
        ritz(going)                 one Rayleigh-Ritz step on each -> {m: (status, evals)}; status WAFER_OK, or WAFER_ERR_STATE where the
                                    states have become linearly dependent (evals is then ignored)
        residuals(going, theta)     rho of the rotated states with theta[m] = the Ritz energies -> {m: rho}
    Per block: step, Ritz, diff_j = |e_j - e_last_j| (inf in the first block), residuals; a row {"block", "steps", "evals", "diff",
    "rho"} is recorded.  A member is done when max_j diff_j < tolerance -- the reference's stopping rule applied to every state of
    the block; rho is reported and never decides (the semi-implicit step's invariant subspaces are not H's: rho has a floor of
    O(dt V)).  Done members leave `going`.
    -> per member None, or {"status", "message", "blocks", "steps", "evals", "diff", "rho", "rows"}: status BLOCK_CONVERGED (WAFER_OK),
    BLOCK_MAX_BLOCKS (WAFER_ERR_MAX_STEP: max_blocks reached, a status and not an exception) or BLOCK_DEPENDENT (WAFER_ERR_STATE: the
    Ritz step found the states linearly dependent; the message says to shorten steps_per_block)."""
    ks = [0 if x is None else int(x) for x in k]
    steps_per_block, max_blocks, tolerance = int(steps_per_block), int(max_blocks), float(tolerance)
    if steps_per_block < 1 or max_blocks < 1:
        raise ValueError("steps_per_block and max_blocks must be >= 1")
    if not tolerance > 0.0:
        raise ValueError("tolerance must be > 0")

    def advance(going, block, out):
        step(list(going), steps_per_block)
        return going

    return _solve_loop(ks, tolerance, steps_per_block, max_blocks, advance, ritz, residuals, lambda o, m: float(np.max(o["diff"])),
                       "member %d: after block %d (%d steps) the Ritz step found the %d states linearly dependent: every state has "
                       "collapsed onto the lowest ones; shorten steps_per_block (now %d)",
                       "member %d: max_blocks = %d reached with max diff %g >= tolerance %g")


# ---- Chebyshev-filtered subspace iteration on the state stores ---------------------------------------------------------------------
FILTER_MAX_DEGREE = 256
FILTER_CONVERGED, FILTER_MAX_BLOCKS, FILTER_DEPENDENT, FILTER_NO_INTERVAL = WAFER_OK, WAFER_ERR_MAX_STEP, WAFER_ERR_STATE, WAFER_ERR_INVALID


def filter_coefficients(degree: int, a: float, b: float, a0: float):
    """(al, be, cc): wafer_filter_coefficients -- host only, no GPU: the `degree` steps' coefficients of the scaled Chebyshev filter
    that damps [a, b] and has magnitude 1 at a0 < a"""
    L = load_library()
    n = max(int(degree), 1)
    al, be, cc = np.zeros(n), np.zeros(n), np.zeros(1)
    rc = L.wafer_filter_coefficients(int(degree), float(a), float(b), float(a0), _dp(al), _dp(be), _dp(cc))
    if rc != 0:
        raise WaferError(rc, L.wafer_last_error().decode())
    return al, be, float(cc[0])


def filtered_solve_loop(bound, filt, ritz, residuals, k, tolerance: float, degree: int, max_blocks: int, guard: int = 1) -> list:
    """Chebyshev-filtered subspace iteration over a set of members, backend-free (Context.solve_filtered, Batch.solve_filtered and the
    numpy model of the tests all call this; block_solve_loop's sibling: its step callable is not told the last Ritz values).  k: one
    state count per member (0 or None: the member takes no part); k[m] - guard >= 1.  Four callables over the members still `going`:
        bound(going)                an upper bound of H's spectrum -> {m: ub}
        filt(going, degree, iv)     applies the degree-`degree` filter with iv[m] = (a, b, a0) to the first k[m] stored states
        ritz(going)                 one Rayleigh-Ritz step on each -> {m: (status, evals)}; WAFER_ERR_STATE where it fails
        residuals(going, theta)     rho of the rotated states with theta[m] = the Ritz values -> {m: rho}
    One Ritz step on the starts; then per block and member a0 = evals[0], a = evals[k - 1], b = ub, the filter, Ritz, residuals; a
    row {"block", "steps" (filter steps so far), "evals", "diff", "rho"}.  A member is done when rho_j < tolerance for the first
    k - guard states: the polynomial is in H, so the fixed points are H's eigenvectors and rho decides.  The guard states are never
    waited for: their gap to the damped interval [evals[k - 1], ub] is zero by construction.
    -> per member None, or {"status", "message", "blocks", "steps", "evals", "diff", "rho", "rows"}: FILTER_CONVERGED (WAFER_OK),
    FILTER_MAX_BLOCKS (WAFER_ERR_MAX_STEP), FILTER_DEPENDENT (WAFER_ERR_STATE: Ritz found the states non-finite or dependent; the
    message says to lower `degree`) or FILTER_NO_INTERVAL (WAFER_ERR_INVALID: evals[k - 1] <= evals[0], or evals[k - 1] >= ub)."""
    ks = [0 if x is None else int(x) for x in k]
    degree, max_blocks, tolerance, guard = int(degree), int(max_blocks), float(tolerance), int(guard)
    if degree < 1 or degree > FILTER_MAX_DEGREE or max_blocks < 1:
        raise ValueError("degree must be 1 .. %d and max_blocks >= 1" % FILTER_MAX_DEGREE)
    if not tolerance > 0.0:
        raise ValueError("tolerance must be > 0")
    if guard < 1 or any(n > 0 and n - guard < 1 for n in ks):
        raise ValueError("guard must be >= 1 and every k - guard >= 1")
    ub = {}

    def advance(going, block, out):
        """the interval gate, then the filter on the members that have one"""
        iv, ready = {}, []
        for m in going:
            e = out[m]["evals"]
            if not e[-1] > e[0]:
                out[m]["status"] = FILTER_NO_INTERVAL
                out[m]["message"] = "member %d: block %d: evals[%d] = %r <= evals[0] = %r: no interval to damp" % (m, block, ks[m] - 1, e[-1], e[0])
            elif not e[-1] < ub[m]:
                out[m]["status"] = FILTER_NO_INTERVAL
                out[m]["message"] = "member %d: block %d: evals[%d] = %r >= the spectral bound %r" % (m, block, ks[m] - 1, e[-1], ub[m])
            else:
                iv[m] = (float(e[-1]), float(ub[m]), float(e[0]))
                ready.append(m)
        if ready:
            filt(list(ready), degree, iv)
        return ready

    return _solve_loop(ks, tolerance, degree, max_blocks, advance, ritz, residuals, lambda o, m: float(np.max(o["rho"][:ks[m] - guard])),
                       "member %d: after block %d (%d filter steps) the Ritz step found the %d states non-finite or linearly "
                       "dependent: lower degree (now %d)",
                       "member %d: max_blocks = %d reached with max rho %g >= tolerance %g", first=lambda going: ub.update(bound(going)))


def _ritz_status(fn):
    """the loops' ritz callable on one member (index 0): fn() -> its Ritz values, where WAFER_ERR_STATE is the member's status and not
    an exception"""
    try:
        return {0: (WAFER_OK, fn())}
    except WaferError as e:
        if e.code != WAFER_ERR_STATE:
            raise
        return {0: (WAFER_ERR_STATE, None)}


class Context:
    """Device-resident solver state for one grid (or one z-slab of it)."""

    def __init__(self, params: Params):
        self._L = load_library()
        self.params = params
        self._h = C.c_void_p()
        p = params.c()
        self._check(self._L.wafer_ctx_create(C.byref(p), C.byref(self._h)))
        self._hooks = None

    # -- plumbing -----------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != WAFER_OK:
            raise WaferError(rc, self._L.wafer_last_error().decode())

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.wafer_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def synchronize(self) -> None:
        self._check(self._L.wafer_synchronize(self._h))

    # -- Potentials (potential.rs:16-25, 75-175) --------------------------------------
    def set_potential(self, name: str) -> None:
        self._check(self._L.wafer_set_potential_builtin(self._h, POTENTIALS.index(name)))

    def set_potential_host(self, v: np.ndarray, potsub_kind: int = 0, potsub_scalar: float = 0.0,
                           potsub: np.ndarray | None = None) -> None:
        assert v.shape == self.params.padded_shape
        self._check(self._L.wafer_set_potential_host(
            self._h, _dp(v), potsub_kind, potsub_scalar, _dp(potsub) if potsub is not None else None))

    def download_array(self, which: str) -> np.ndarray:
        idx = {"v": 0, "a": 1, "b": 2, "potsub": 3}[which]
        out = np.zeros(self.params.work_shape if which == "potsub" else self.params.padded_shape)
        self._check(self._L.wafer_download_array(self._h, idx, _dp(out)))
        return out

    def download_window(self, which: str, zp_begin: int, zp_count: int) -> np.ndarray:
        """global padded planes [zp_begin, zp_begin + zp_count) of "v" / "a" / "b" / "phi" in the reference's layout:
        (px, py, zp_count) -- download_array / download_phi restricted to a z-window (wafer_diag_download_window)"""
        px, py, _ = self.params.padded_shape
        out = np.zeros((px, py, zp_count))
        self._check(self._L.wafer_diag_download_window(self._h, {"v": 0, "a": 1, "b": 2, "phi": 4}[which], zp_begin, zp_count, _dp(out)))
        return out

    def set_potsub(self, kind: int, scalar: float = 0.0, potsub: np.ndarray | None = None) -> None:
        """override pot_sub (a potential_sub file in ./input, potential.rs:113-131)"""
        if potsub is not None:
            assert potsub.shape == self.params.work_shape
        self._check(self._L.wafer_set_potsub(self._h, kind, scalar, _dp(potsub) if potsub is not None else None))

    def set_potsub_resampled(self, src: np.ndarray) -> None:
        """pot_sub from an array of another resolution (input::fill_sub_data, input.rs:453-478)"""
        src = np.ascontiguousarray(src, dtype=np.float64)
        assert src.ndim == 3
        self._check(self._L.wafer_set_potsub_resampled(self._h, _dp(src), *src.shape))

    def potsub(self):
        kind, scalar = C.c_int(0), C.c_double(0.0)
        self._check(self._L.wafer_get_potsub(self._h, C.byref(kind), C.byref(scalar)))
        return kind.value, scalar.value

    # -- phi ----------------------------------------------------------------------------
    def set_initial_condition(self, name: str, seed: int = 0) -> None:
        self._check(self._L.wafer_set_initial_condition(self._h, INITIAL_CONDITIONS.index(name), seed))

    def symmetrise(self, constraint: str) -> None:
        """config::symmetrise_wavefunction (config.rs:691-728); SevenPoint only, like the reference"""
        self._check(self._L.wafer_symmetrise(self._h, SYMMETRY.index(constraint)))

    def div_check(self, den: float, n_operands: int, lo_exp: int = 64, hi_exp: int = 1983, seed: int = 1) -> int:
        """operands (of n_operands random ones) whose hoisted-reciprocal quotient by `den` differs from the
        IEEE division in any bit (wafer_diag_div_check)"""
        bad = C.c_uint64(0)
        self._check(self._L.wafer_diag_div_check(self._h, den, seed, n_operands, lo_exp, hi_exp, C.byref(bad)))
        return int(bad.value)

    def div_plan(self) -> _DivPlan:
        """the plan of x / (c dn^2 m) this context's kernels run with (wafer_get_div_plan)"""
        p = _DivPlan()
        self._check(self._L.wafer_get_div_plan(self._h, C.byref(p)))
        return p

    def div_planned_check(self, plan: _DivPlan, n_random: int = 0, operands=None, lo_exp: int = 64, hi_exp: int = 1983, seed: int = 1):
        """(mismatches among n_random drawn operands, mismatches among `operands`): the planned division as the kernels perform
        it against the device's IEEE x / den, bit for bit (wafer_diag_div_planned)"""
        ops = np.ascontiguousarray(operands, dtype=np.float64) if operands is not None else np.zeros(0)
        bad_r, bad_o = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_diag_div_planned(self._h, C.byref(plan), seed, n_random, lo_exp, hi_exp,
                                                   _dp(ops) if ops.size else None, ops.size, C.byref(bad_r), C.byref(bad_o)))
        return int(bad_r.value), int(bad_o.value)

    def div_planned_check_f32(self, plan: _DivPlanF32, lo_exp: int = 27, hi_exp: int = 227) -> int:
        """floats (ALL significands, both signs, biased exponents lo_exp .. hi_exp) whose planned fp32 quotient differs from the
        device's IEEE x / den in any bit (wafer_diag_div_planned_f32)"""
        bad = C.c_uint64(0)
        self._check(self._L.wafer_diag_div_planned_f32(self._h, C.byref(plan), lo_exp, hi_exp, C.byref(bad)))
        return int(bad.value)

    def download_phi_owned(self) -> np.ndarray:
        """the work cells of the planes this context owns, (nx, ny, z_count)"""
        p = self.params
        out = np.zeros((p.nx, p.ny, p.z_count if p.z_count else p.nz))
        self._check(self._L.wafer_download_phi_owned(self._h, _dp(out)))
        return out

    def upload_phi(self, phi: np.ndarray) -> None:
        assert phi.shape == self.params.padded_shape
        self._check(self._L.wafer_upload_phi(self._h, _dp(phi)))

    @staticmethod
    def _basis(basis):
        return None if basis is None else (C.c_uint32 * 3)(*basis)

    def upload_phi_resampled(self, src: np.ndarray, basis=None) -> None:
        """input.rs:667-716: trilinear resample of an unpadded array of another resolution"""
        self._check(self._L.wafer_upload_phi_resampled(self._h, _dp(src), *src.shape, self._basis(basis)))

    def set_potential_resampled(self, src: np.ndarray, basis=None) -> None:
        self._check(self._L.wafer_set_potential_resampled(self._h, _dp(src), *src.shape, self._basis(basis)))

    def download_phi(self, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros(self.params.padded_shape)
        self._check(self._L.wafer_download_phi(self._h, _dp(out)))
        return out

    # -- hot path (grid.rs) ---------------------------------------------------------------
    def evolve(self, wnum: int, steps: int) -> None:
        """grid.rs:544-687"""
        self._check(self._L.wafer_evolve(self._h, wnum, steps))

    def observables(self) -> dict:
        """grid.rs:303-445 (un-normalised)"""
        o = _Obs()
        self._check(self._L.wafer_observables(self._h, C.byref(o)))
        return dict(energy=o.energy, norm2=o.norm2, v_infinity=o.v_infinity, r2=o.r2)

    def norm2(self) -> float:
        """grid.rs:454-457"""
        v = C.c_double(0.0)
        self._check(self._L.wafer_norm2(self._h, C.byref(v)))
        return v.value

    def normalise(self, norm2: float) -> None:
        """grid.rs:465-468"""
        self._check(self._L.wafer_normalise(self._h, norm2))

    def orthogonalise(self, wnum: int) -> None:
        """grid.rs:477-492"""
        self._check(self._L.wafer_orthogonalise(self._h, wnum))

    # -- w_store ---------------------------------------------------------------------------
    def push_state(self) -> None:
        self._check(self._L.wafer_push_state(self._h))

    def load_state(self, idx: int, state: np.ndarray) -> None:
        assert state.shape == self.params.padded_shape
        self._check(self._L.wafer_load_state(self._h, idx, _dp(state)))

    def download_state(self, idx: int) -> np.ndarray:
        out = np.zeros(self.params.padded_shape)
        self._check(self._L.wafer_download_state(self._h, idx, _dp(out)))
        return out

    def clone_state_to_phi(self, idx: int) -> None:
        self._check(self._L.wafer_clone_state_to_phi(self._h, idx))

    def num_states(self) -> int:
        n = C.c_uint32(0)
        self._check(self._L.wafer_num_states(self._h, C.byref(n)))
        return n.value

    def clear_states(self) -> None:
        self._check(self._L.wafer_clear_states(self._h))

    # -- Rayleigh-Ritz on w_store (include/wafer_hip.h) ------------------------------------------------
    def _ritz_k(self, k) -> int:
        return self.num_states() if k is None else int(k)

    def ritz_matrices(self, k: int | None = None):
        """-> (h, s), (k, k) each: h[j, i] = sum l_i (H l_j), s[j, i] = sum l_i l_j over the first k stored states (all of them
        when k is None)"""
        k = self._ritz_k(k)
        h, s = np.zeros((max(k, 1), max(k, 1))), np.zeros((max(k, 1), max(k, 1)))
        self._check(self._L.wafer_ritz_matrices(self._h, k, _dp(h), _dp(s)))
        return h, s

    def moments(self, k: int | None = None) -> dict:
        """-> {"s", "x", "y", "z", "r2": (k, k) each, "origin": (cx, cy, cz)}: <l_i|q|l_j> over the first k stored states (all of them
        when k is None) for q = 1, x - cx, y - cy, z - cz and their squares' sum, in index units, from one sums launch.  The origin is
        observables' own, (n + 1) / 2 per axis in 0-based work indices -- one cell above the geometric centre; <i|x - c|j> =
        x[i, j] - (c - cx) * s[i, j] moves it.  r2[j, j] and s[j, j] have the bits of observables()'s r2 and norm2 on state j.
        Read-only; needs no potential."""
        k = self._ritz_k(k)
        m = np.zeros((MOMENT_COUNT, max(k, 1), max(k, 1)))
        self._check(self._L.wafer_moment_matrices(self._h, k, _dp(m)))
        out = {name: m[q].copy() for q, name in enumerate(MOMENT_NAMES)}
        out["origin"] = moment_origin(self.params.nx, self.params.ny, self.params.nz)
        return out

    def rotate_states(self, coef: np.ndarray) -> None:
        """l'_a = sum_j coef[j, a] l_j for the first k = len(coef) stored states, in place"""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[0] != coef.shape[1]:
            raise ValueError(f"coef must be a square matrix, not {coef.shape}")
        self._check(self._L.wafer_rotate_states(self._h, coef.shape[0], _dp(coef)))

    def ritz(self, k: int | None = None) -> dict:
        """matrices, solve, rotate -> {"evals": (k,), "coef": (k, k), "h": (k, k), "s": (k, k)}; h, s are those before the rotation"""
        k = self._ritz_k(k)
        n = max(k, 1)
        evals, coef, h, s = np.zeros(n), np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
        self._check(self._L.wafer_ritz(self._h, k, _dp(evals), _dp(coef), _dp(h), _dp(s)))
        return {"evals": evals, "coef": coef, "h": h, "s": s}

    # -- stepping w_store: subspace iteration (include/wafer_hip.h) --------------------------------------
    def evolve_states(self, k: int, steps: int) -> None:
        """the first k stored states advanced by `steps` plain steps each (no projection, no normalisation): every one holds the
        bits of clone_state_to_phi(j); evolve(0, steps).  phi and the current buffer are left alone."""
        self._check(self._L.wafer_evolve_states(self._h, int(k), int(steps)))

    def seed_states(self, k: int, seed: int) -> None:
        """k fresh stored states: the Gaussian initial condition with seed + j, pushed, for j = 0 .. k-1.  OVERWRITES phi (it holds
        the last of them afterwards); the store is not cleared first."""
        for j in range(int(k)):
            self.set_initial_condition("Gaussian", int(seed) + j)
            self.push_state()

    def solve_block(self, k: int, tolerance: float, steps_per_block: int, max_blocks: int) -> dict:
        """Subspace iteration on the first k stored states (block_solve_loop): evolve_states(k, steps_per_block), ritz(k), the Ritz
        energies against the last block's, residuals(k, theta=evals) -- until every |e_j - e_last_j| < tolerance.
        -> {"status", "message", "blocks", "steps", "evals", "diff", "rho", "rows"}"""
        k = int(k)
        return block_solve_loop(lambda going, n: self.evolve_states(k, n), lambda going: _ritz_status(lambda: self.ritz(k)["evals"]),
                                lambda going, theta: {0: self.residuals(k, theta=theta[0])["rho"]}, [k], tolerance, steps_per_block, max_blocks)[0]

    # -- filtering w_store: Chebyshev-filtered subspace iteration (include/wafer_hip.h) ------------------
    def filter_states(self, k: int, degree: int, a: float, b: float, a0: float) -> None:
        """the degree-`degree` scaled Chebyshev polynomial of H that damps [a, b] and has magnitude 1 at a0 < a, applied to the first k
        stored states (one launch per state and step).  phi and the current buffer are left alone."""
        self._check(self._L.wafer_filter_states(self._h, int(k), int(degree), float(a), float(b), float(a0)))

    def spectral_bound(self) -> float:
        """Gershgorin's upper bound of H's spectrum: W / den + max V over the work cells"""
        ub = np.zeros(1)
        self._check(self._L.wafer_spectral_bound(self._h, _dp(ub)))
        return float(ub[0])

    def solve_filtered(self, k: int, tolerance: float, degree: int, max_blocks: int, guard: int = 1) -> dict:
        """Chebyshev-filtered subspace iteration on the first k stored states (filtered_solve_loop): ritz(k), then per block
        filter_states(k, degree, evals[k - 1], spectral_bound(), evals[0]), ritz(k), residuals(k, theta=evals) -- until rho < tolerance
        on the first k - guard states.  -> {"status", "message", "blocks", "steps", "evals", "diff", "rho", "rows"}"""
        k = int(k)
        return filtered_solve_loop(lambda going: {0: self.spectral_bound()}, lambda going, n, iv: self.filter_states(k, n, *iv[0]),
                                   lambda going: _ritz_status(lambda: self.ritz(k)["evals"]),
                                   lambda going, theta: {0: self.residuals(k, theta=theta[0])["rho"]}, [k], tolerance, degree, max_blocks, guard)[0]

    # -- residuals of w_store and of phi (include/wafer_hip.h) -------------------------------------------
    def residuals(self, k: int | None = None, theta=None, source: str = "states") -> dict:
        """r = H l - theta l of the first k stored states (all of them when k is None), or of phi (source="phi", k = 1):
        {"theta": (k,), "r2": (k,) sum r^2, "norm2": (k,) sum l^2, "rho": (k,) sqrt(r2 / norm2)} -- some eigenvalue of the discrete
        H lies within rho[j] of theta[j].  theta: k values, or None for each source's Rayleigh quotient (a second pass).  Read-only."""
        if source not in RESIDUAL_SOURCES:
            raise ValueError("source must be 'states' or 'phi', not %r" % (source,))
        k = (1 if source == "phi" else self.num_states()) if k is None else int(k)
        if not 1 <= k <= RITZ_MAX:
            raise ValueError("k = %d is outside 1 .. RITZ_MAX = %d" % (k, RITZ_MAX))
        if source == "phi" and k != 1:
            raise ValueError("k = %d: the phi source is one array (k = 1)" % k)
        tin = None
        if theta is not None:
            tin = np.ascontiguousarray(np.atleast_1d(theta), dtype=np.float64)
            if tin.shape != (k,):
                raise ValueError("theta must hold k = %d values, not shape %s" % (k, tin.shape))
            if not np.all(np.isfinite(tin)):
                raise ValueError("theta must be finite")
        th, r2, s = np.zeros(k), np.zeros(k), np.zeros(k)
        self._check(self._L.wafer_residuals(self._h, RESIDUAL_SOURCES[source], k, None if tin is None else _dp(tin), _dp(th), _dp(r2), _dp(s)))
        return {"theta": th, "r2": r2, "norm2": s, "rho": np.sqrt(r2 / s)}

    def residual_to_phi(self, idx: int, theta: float) -> None:
        """phi = H l - theta l of stored state idx (zeros outside the work area); the store is left alone"""
        theta = float(theta)
        if not np.isfinite(theta):
            raise ValueError("theta must be finite")
        self._check(self._L.wafer_residual_to_phi(self._h, int(idx), theta))

    # -- solve (grid.rs:50-246) --------------------------------------------------------------
    def solve_state(self, wnum: int, tolerance: float, screen_update: int, max_steps=None,
                    max_records: int = 100000):
        """-> (records, final, converged).  Raises on errors other than MaxStep."""
        recs = (_Record * max_records)()
        n = C.c_size_t(0)
        fin = _ObsOut()
        rc = self._L.wafer_solve_state(self._h, wnum, tolerance, screen_update,
                                       0 if max_steps is None else 1,
                                       0 if max_steps is None else int(max_steps), recs, max_records,
                                       C.byref(n), C.byref(fin))
        if rc not in (WAFER_OK, WAFER_ERR_MAX_STEP):
            self._check(rc)
        out = []
        for i in range(min(n.value, max_records)):
            r = recs[i]
            out.append(dict(step=r.step, tau=r.tau, energy=r.obs.energy, norm2=r.obs.norm2,
                            v_infinity=r.obs.v_infinity, r2=r.obs.r2, diff=r.diff))
        final = dict(state=fin.state, energy=fin.energy, binding_energy=fin.binding_energy,
                     r=fin.r, l_r=fin.l_r)
        return out, final, rc == WAFER_OK

    # -- measurement ----------------------------------------------------------------------------
    def last_evolve_ms(self):
        ms, steps = C.c_float(0.0), C.c_uint64(0)
        self._check(self._L.wafer_last_evolve_ms(self._h, C.byref(ms), C.byref(steps)))
        return ms.value, steps.value

    def stencil_kernel_name(self) -> str:
        return self._L.wafer_stencil_kernel_name(self._h).decode()

    def stencil_kernel_instance(self) -> str:
        """template-id of the kernel the last ground-state pass launched, as a profiler prints it"""
        return self._L.wafer_stencil_kernel_instance(self._h).decode()

    def steps_per_launch(self) -> int:
        return int(self._L.wafer_stencil_steps_per_launch(self._h))

    def set_stencil_variant(self, variant: int) -> None:
        self._check(self._L.wafer_set_stencil_variant(self._h, variant))

    def copy_bandwidth(self, iters: int = 50, unroll: int = 4, blocks_per_cu: int = 1) -> float:
        """measured GB/s (read + written) of a 16 B-per-lane device copy: the device's own ceiling"""
        v = C.c_double(0.0)
        self._check(self._L.wafer_diag_copy_bw(self._h, iters, unroll, blocks_per_cu, C.byref(v)))
        return v.value

    def dispatch(self, wnum: int = 0) -> dict:
        """which kernel a pass of evolve(wnum, .) launches for this context (wafer_diag_dispatch): {"kernel": ..., "steps_per_pass": ...,
        "ghost_planes_per_pass": ..., "tile": ..., "v": "streamed" | "closed_form", ...} -- the launch path's own predicates"""
        buf = C.create_string_buffer(512)
        self._check(self._L.wafer_diag_dispatch(self._h, wnum, buf, len(buf)))
        out = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        for k in ("wnum", "stencil", "steps_per_pass", "ghost_planes_per_pass", "nlow", "waves"):
            if k in out:
                out[k] = int(out[k])
        return out

    def x2_passes(self) -> int:
        """passes of the two-excited-steps-per-pass kernel launched so far (include/wafer_hip.h)"""
        v = C.c_uint64(0)
        self._check(self._L.wafer_diag_x2_passes(self._h, C.byref(v)))
        return int(v.value)

    def checksum(self, z_begin: int = 0, z_count: int | None = None) -> int:
        """position-dependent integer checksum of the owned work cells of global planes
        [z_begin, z_begin + z_count): equal bits <=> equal checksums, whatever the decomposition"""
        v = C.c_uint64(0)
        n = self.params.nz if z_count is None else z_count
        self._check(self._L.wafer_diag_checksum(self._h, z_begin, n, C.byref(v)))
        return int(v.value)

    # -- multi-GPU ---------------------------------------------------------------------------------
    def set_comm_hooks(self, halo, allreduce) -> None:
        """halo(send_lo, send_hi, recv_lo, recv_hi, nbytes, stream) and
        allreduce(dev_ptr, count, stream): python callables taking raw device
        addresses (ints or None); they must return 0 on success."""
        def _halo(_user, slo, shi, rlo, rhi, nbytes, stream):
            try:
                return int(halo(slo, shi, rlo, rhi, nbytes, stream) or 0)
            except Exception as e:  # never unwind through C
                print("wafer halo hook failed:", repr(e), flush=True)
                return 1

        def _allreduce(_user, ptr, count, stream):
            try:
                return int(allreduce(ptr, count, stream) or 0)
            except Exception as e:
                print("wafer allreduce hook failed:", repr(e), flush=True)
                return 1

        self._hooks = (HALO_FN(_halo), ALLREDUCE_FN(_allreduce))  # keep alive
        self._check(self._L.wafer_set_comm_hooks(self._h, self._hooks[0], self._hooks[1], None))

    def peer_export(self) -> bytes:
        """this context's wafer_peer_info record (for the z-neighbours' peer_connect), as bytes any transport can carry"""
        info = _PeerInfo()
        self._check(self._L.wafer_peer_export(self._h, C.byref(info)))
        return bytes(info)

    def peer_connect(self, lower: bytes | None, upper: bytes | None) -> None:
        """map the z-neighbours' buffers and arrival counters (records from their peer_export; None: no neighbour on that side):
        the precondition of set_overlap(3)"""
        recs = [_PeerInfo.from_buffer_copy(r) if r is not None else None for r in (lower, upper)]
        self._check(self._L.wafer_peer_connect(self._h, C.byref(recs[0]) if recs[0] is not None else None,
                                               C.byref(recs[1]) if recs[1] is not None else None))

    def peer_disconnect(self) -> None:
        self._check(self._L.wafer_peer_disconnect(self._h))

    def set_overlap(self, enabled) -> None:
        """halo schedule of a z-slab: False / 0 (exchange after the pass), True / 1 (boundary planes first, three launches
        per pass), 2 (the default: one launch per three-step pass, exchanges released by completion counters), 3 (the same
        launch with peer stores into the neighbours' ghost planes instead of an exchange: after peer_connect);
        include/wafer_hip.h"""
        self._check(self._L.wafer_set_overlap(self._h, int(enabled)))

    def set_halo_cycle(self, passes: int) -> None:
        """fused passes per halo exchange of a z-slab (needs halo_depth >= K * ext * passes, K = steps per fused pass)"""
        self._check(self._L.wafer_set_halo_cycle(self._h, int(passes)))

    def set_stream(self, stream_ptr: int | None) -> None:
        self._check(self._L.wafer_set_stream(self._h, stream_ptr))

    def device_info(self) -> dict:
        d = _DeviceInfo()
        self._check(self._L.wafer_get_device_info(self._h, C.byref(d)))
        out = {k: getattr(d, k) for k, _ in _DeviceInfo._fields_}
        out["name"], out["arch"] = d.name.decode(), d.arch.decode()
        return out

    def slab_info(self) -> dict:
        s = _SlabInfo()
        self._check(self._L.wafer_get_slab_info(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _SlabInfo._fields_}


class Batch:
    """B independent problems of one shape on one device (wafer_batch_*): one launch per step advances every active member,
    and each member's ground state computes bit for bit what a Context with its Params computes.  set_step_variant(1) makes
    a ground-state evolve one launch per pass of K steps (ThreePoint 3, FivePoint 2; steps_per_launch(), dispatch()): the
    same bits.

    dtype: every member's Params.dtype must be the same -- "f64", "f32" (float arrays, fp64 arithmetic) or "f32fast" (float
    arithmetic in the ground-state step too).  On the float dtypes the arrays and state stores take half the bytes per cell, numpy
    arrays stay float64 (uploads and load_state round to float, downloads widen), the ground state, observables, normalise
    and solve are bit for bit a Context of that dtype (every step's result rounded to float, under fused passes as well), and
    the excited-state calls compute in fp64 with phi rounded to float after the step, the scale and each projection.

    Excited states: every member has a state store of its own (capacity Params.max_states; load_state, push_state, ...), and
    evolve(steps, wnum=k) / solve_state(k, ...) normalise and project each member against its first k stored states after
    every step, as Context.evolve(k, steps) does, in 1 + 2 (1 + k) + 1 launches per step for the whole batch.  A member's
    bits do not depend on the batch size, its index or the active set; against a Context they agree to the excited-state
    tolerances (1e-13 per cell), not bit for bit: the sums are partitioned differently.  Measured (ThreePoint
    fp64, 50^3 and 64^3, wnum 1 and 2): 1.7-3.2 times B contexts one after another from B = 8 on, 0.4 times at B = 1 -- for one
    problem use a Context.
    set_gs_variant(1) selects the one-pass form for wnum <= 4 (opt-in): step, raw sums, reduce and one apply pass with the
    member's Gram matrix, 4 launches per step whatever k and B; the same tolerances against the oracle and a Context, phi rounded
    to float once per step on the float dtypes, not the sequential form's bits (gs_dispatch(wnum), gs_steps()).
    A sweep over states is solve_state(0), solve_state(1), ...: a member whose store is too short for a call gets the status
    WAFER_ERR_STATE, is left as it is, and the others run.

    mixed_shapes=True (wafer_batch_create_mixed): the members' nx, ny, nz may differ -- a convergence study in one batch.  The
    ground-state path (evolve with wnum = 0 under both step variants, observables, norm2, normalise, solve) gives every member the
    bits of a Context of its own Params on every dtype (but norm2 on f64: the Context's partition of that sum is another, and the
    two agree to 1e-12), in one launch per step or pass for all shapes together (num_shapes(), dispatch()["shapes"]).  With more than one distinct shape the calls that need the state stores (load_state, download_state,
    push_state, clear_states, clone_state_to_phi, orthogonalise, evolve with wnum > 0, solve_state, set_gs_variant(1)) raise
    WaferError -1 with "mixed-shape" in the message; with one distinct shape the batch is a plain Batch in every call.
    mixed_shapes=True, state_stores=True (wafer_batch_create_mixed_states) lifts that: every state-store and excited-state call
    works on several shapes, in the same number of launches per step for all shapes together, and gives each member bit for bit
    what it gets in a Batch of its own shape under the same gs variant, on every dtype (gs_dispatch(wnum)["shapes"]).
    state_stores=True without mixed_shapes=True is a ValueError: a Batch of one shape always has its stores.

    symmetrise(constraints, active=None) applies constraints[m] (a name of SYMMETRY or its index, one per member) to every active
    member in ONE launch, each member bit for bit what Context.symmetrise gives, on one shape and on several; members that are
    inactive or "NotConstrained" keep their buffer and their bits.  SevenPoint only, like a Context, unless every constraint is
    "NotConstrained".  set_potsub(i, kind, scalar, potsub) is Context.set_potsub for member i (a potential_sub override).
    resample_phi / resample_potential / resample_potsub / resample_state(idx, ...) set an array of every active member from ONE source
    of any resolution in one launch (wafer_k_batch_trilerp): a numpy array, uploaded once, or ("member", m) / ("state", m, l), the work
    cells of member m's phi or stored state l on the device -- a coarse member's result as the start of a finer one.  Each member gets
    bit for bit what Context.upload_phi_resampled / set_potential_resampled / set_potsub_resampled give a Context of its Params
    (basis "padded": the reference's production call; "work": its nx, ny, nz), with that call's bookkeeping; resample_state follows
    load_state's rules.  A refused call changes nothing.
    set_potentials(names, active) / set_initial_conditions(names, seeds, active) set every listed member up in one launch each --
    with ONE range check and read-back for all of them where a per-member call pays two launches, two read-backs and a synchronisation
    each -- bit for bit what set_potential / set_initial_condition give member by member (setup_counts()).  download_array(i, which),
    potsub(i) and member_info(i) read a member back as a Context's calls do.
    ritz_matrices(k, active) / rotate_states(coefs, active) / ritz(k, active): Context.ritz_matrices / rotate_states / ritz on the first
    k[m] stored states of every listed member -- one sums launch, one reduce and one read-back for all members of any shapes, the
    solves on the host, one rotation launch for the members that solved (ritz_counts()) -- each member bit for bit what a Context of
    its Params with the same potential and states gets.  k: an int, one entry per member, or None for each member's state count.  A
    member whose solve fails keeps its store and reports it in its "status"; the others are rotated.
    residuals(k, theta, active, source): Context.residuals for every listed member -- theta and rho = |H l - theta l| / |l| of its first
    k[m] stored states, or of its phi on any batch (source="phi") -- one sums launch, one reduce and one read-back per pass for all
    members of any shapes (residual_counts()), each member its Context's bits; read-only.
    python -m wafer_amd.sweep drives whole wafer.yaml runs through batches with these calls: phases per state number, every run
    with its own screen_update, tolerance and max_steps, one evolve for all running members between block boundaries."""

    def __init__(self, members: list, mixed_shapes: bool = False, state_stores: bool = False):
        if state_stores and not mixed_shapes:
            raise ValueError("state_stores=True goes with mixed_shapes=True (a Batch of one shape always has state stores)")
        self._L = load_library()
        self.members = list(members)
        self._h = C.c_void_p()
        arr = (_Params * max(1, len(self.members)))(*[m.c() for m in self.members])
        create = self._L.wafer_batch_create
        if mixed_shapes:
            create = self._L.wafer_batch_create_mixed_states if state_stores else self._L.wafer_batch_create_mixed
        self._check(create(arr, len(self.members), C.byref(self._h)))

    def _check(self, rc: int) -> None:
        if rc != WAFER_OK:
            raise WaferError(rc, self._L.wafer_last_error().decode())

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.wafer_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self) -> int:
        return len(self.members)

    def num_shapes(self) -> int:
        """distinct (nx, ny, nz) among the members"""
        n = C.c_uint32(0)
        self._check(self._L.wafer_batch_num_shapes(self._h, C.byref(n)))
        return n.value

    def _mask(self, active):
        if active is None:
            return None
        a = np.ascontiguousarray(np.asarray(active, dtype=np.uint8))
        if a.shape != (len(self.members),):
            raise ValueError("active must hold one entry per member")
        return a

    @staticmethod
    def _u8(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))

    # -- set-up, per member --------------------------------------------------------------
    def set_potential(self, i: int, name: str) -> None:
        self._check(self._L.wafer_batch_set_potential_builtin(self._h, i, POTENTIALS.index(name)))

    def set_potential_host(self, i: int, v: np.ndarray, potsub_kind: int = 0, potsub_scalar: float = 0.0,
                           potsub: np.ndarray | None = None) -> None:
        assert v.shape == self.members[i].padded_shape
        self._check(self._L.wafer_batch_set_potential_host(
            self._h, i, _dp(v), potsub_kind, potsub_scalar, _dp(potsub) if potsub is not None else None))

    def set_potsub(self, i: int, kind: int, scalar: float = 0.0, potsub: np.ndarray | None = None) -> None:
        """override member i's pot_sub after its potential is set (Context.set_potsub: 0 none, 1 scalar, 2 array of the work shape)"""
        i = self._member(i)
        if potsub is not None:
            assert potsub.shape == self.members[i].work_shape
        self._check(self._L.wafer_batch_set_potsub(self._h, i, kind, scalar, _dp(potsub) if potsub is not None else None))

    def set_initial_condition(self, i: int, name: str, seed: int = 0) -> None:
        self._check(self._L.wafer_batch_set_initial_condition(self._h, i, INITIAL_CONDITIONS.index(name), seed))

    # -- set-up, many members in one launch --------------------------------------------------------
    def set_potentials(self, names, active=None) -> None:
        """Batch.set_potential(m, names[m]) for every listed member (active[m] != 0; None: all) at once: one launch that generates V,
        one for the pot_sub arrays if a listed member is FullCornell, one range check and one read-back for all of them, each member
        bit for bit what the per-member call gives.  names: one per member (a name of POTENTIALS or its index); the entries of
        members not listed are ignored.  A refused call changes nothing."""
        a = self._mask(active)
        pots = _enum_entries(names, POTENTIALS, len(self.members), a, "potential")
        self._check(self._L.wafer_batch_set_potentials_builtin(self._h, self._u8(a), (C.c_int * len(pots))(*pots)))

    def set_initial_conditions(self, names, seeds=None, active=None) -> None:
        """Batch.set_initial_condition(m, names[m], seeds[m]) for every listed member in ONE launch, no read-back (seeds None: 0)"""
        a = self._mask(active)
        ics = _enum_entries(names, INITIAL_CONDITIONS, len(self.members), a, "initial condition")
        if seeds is None:
            seeds = [0] * len(self.members)
        if len(seeds) != len(self.members):
            raise ValueError("seeds must hold one entry per member")
        self._check(self._L.wafer_batch_set_initial_conditions(self._h, self._u8(a), (C.c_int * len(ics))(*ics),
                                                               (C.c_uint64 * len(ics))(*[int(x) for x in seeds])))

    def download_array(self, i: int, which: str) -> np.ndarray:
        """Context.download_array of member i: "v", "a", "b" (padded) or "potsub" (the work shape; only where pot_sub is an array)"""
        i = self._member(i)
        idx = {"v": 0, "a": 1, "b": 2, "potsub": 3}[which]
        out = np.zeros(self.members[i].work_shape if which == "potsub" else self.members[i].padded_shape)
        self._check(self._L.wafer_batch_download_array(self._h, i, idx, _dp(out)))
        return out

    def potsub(self, i: int):
        """(kind, scalar) of member i's pot_sub, as Context.potsub"""
        kind, scalar = C.c_int(0), C.c_double(0.0)
        self._check(self._L.wafer_batch_get_potsub(self._h, self._member(i), C.byref(kind), C.byref(scalar)))
        return kind.value, scalar.value

    def member_info(self, i: int) -> dict:
        """member i's host record (wafer_batch_diag_member): member, have_pot, have_phi, potsub_kind, v_in_range, v_ysym, short_forms,
        cur, states -- all ints; launches nothing"""
        buf = C.create_string_buffer(256)
        self._check(self._L.wafer_batch_diag_member(self._h, self._member(i), buf, len(buf)))
        return {k: int(v) for k, v in (kv.split("=", 1) for kv in buf.value.decode().split())}

    def setup_counts(self) -> tuple:
        """(launches, read-backs) of the batched set-up paths since creation: set_potentials, set_initial_conditions and the one range
        check behind resample_potential"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_setup_counts(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def symmetrise(self, constraints, active=None) -> None:
        """Context.symmetrise for every active member (None: all) in one launch, member m with constraints[m]: a name of SYMMETRY
        or its index.  SevenPoint only unless every constraint is NotConstrained; the other members keep their bits."""
        cons = [SYMMETRY.index(c) if isinstance(c, str) else int(c) for c in constraints]
        if len(cons) != len(self.members):
            raise ValueError("constraints must hold one entry per member")
        a = self._mask(active)
        self._check(self._L.wafer_batch_symmetrise(self._h, self._u8(a), (C.c_int * len(cons))(*cons)))

    # -- resampling: one source onto many members in one launch ---------------------------------
    def _resample(self, target: int, idx: int, src, active, basis) -> None:
        """src: an unpadded 3-d numpy array, ("member", m): the work cells of member m's phi, or ("state", m, l): of its stored state l"""
        a = self._mask(active)
        if basis not in RESAMPLE_BASIS:
            raise ValueError("basis must be one of %s" % (RESAMPLE_BASIS,))
        basis = RESAMPLE_BASIS.index(basis)
        if isinstance(src, tuple):
            if len(src) == 2 and src[0] == "member":
                kind, m, l = RESAMPLE_PHI, src[1], 0
            elif len(src) == 3 and src[0] == "state":
                kind, m, l = RESAMPLE_STATE, src[1], src[2]
            else:
                raise ValueError('a member source is ("member", m) or ("state", m, l)')
            self._check(self._L.wafer_batch_resample_member(self._h, self._u8(a), target, idx, self._member(m), kind, int(l), basis))
            return
        src = np.ascontiguousarray(src, dtype=np.float64)
        if src.ndim != 3:
            raise ValueError("the source must be a 3-d array")
        self._check(self._L.wafer_batch_resample(self._h, self._u8(a), target, idx, _dp(src), *src.shape, basis))

    def resample_phi(self, src, active=None, basis: str = "padded") -> None:
        """Context.upload_phi_resampled(src) for every active member (None: all) in ONE launch from one source, each member bit for
        bit what its Context gets; basis "padded" (the reference's production call) or "work" (the member's nx, ny, nz)"""
        self._resample(RESAMPLE_PHI, 0, src, active, basis)

    def resample_potential(self, src, active=None, basis: str = "padded") -> None:
        """Context.set_potential_resampled(src) for every active member in one launch"""
        self._resample(RESAMPLE_POTENTIAL, 0, src, active, basis)

    def resample_potsub(self, src, active=None, basis: str = "work") -> None:
        """Context.set_potsub_resampled(src) for every active member in one launch (after their potentials; basis "work" only)"""
        self._resample(RESAMPLE_POTSUB, 0, src, active, basis)

    def resample_state(self, idx: int, src, active=None, basis: str = "padded") -> None:
        """stored state idx of every active member from one source, under load_state's rules (idx <= the member's count)"""
        self._resample(RESAMPLE_STATE, int(idx), src, active, basis)

    def last_resample_ms(self) -> float:
        """HIP-event time of the last resample_* call's upload, transpose and launch, in milliseconds"""
        ms = C.c_float(0)
        self._check(self._L.wafer_batch_last_resample_ms(self._h, C.byref(ms)))
        return ms.value

    def upload_phi(self, i: int, phi: np.ndarray) -> None:
        assert phi.shape == self.members[i].padded_shape
        self._check(self._L.wafer_batch_upload_phi(self._h, i, _dp(phi)))

    def download_phi(self, i: int, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros(self.members[i].padded_shape)
        self._check(self._L.wafer_batch_download_phi(self._h, i, _dp(out)))
        return out

    # -- hot path ----------------------------------------------------------------------
    def evolve(self, steps: int, active=None, wnum: int = 0) -> None:
        """`steps` steps of state `wnum` of the active members (None: all); wnum = 0: ground-state steps"""
        a, wnum = self._mask(active), self._wnum(wnum)
        if wnum == 0:
            self._check(self._L.wafer_batch_evolve(self._h, self._u8(a), steps))
        else:
            self._check(self._L.wafer_batch_evolve_state(self._h, self._u8(a), wnum, steps))

    def _wnum(self, wnum) -> int:
        wnum = int(wnum)
        if not 0 <= wnum <= max(m.max_states for m in self.members):
            raise ValueError("wnum %d is outside 0 .. max_states = %d" % (wnum, max(m.max_states for m in self.members)))
        return wnum

    def _member(self, i) -> int:
        i = int(i)
        if not 0 <= i < len(self.members):
            raise ValueError("member %d out of range (the batch has %d)" % (i, len(self.members)))
        return i

    def orthogonalise(self, wnum: int, active=None) -> None:
        """grid.rs:477-492 for the active members, each against its own first `wnum` stored states"""
        a, wnum = self._mask(active), self._wnum(wnum)
        self._check(self._L.wafer_batch_orthogonalise(self._h, self._u8(a), wnum))

    def norm2(self) -> list:
        """grid.rs:454-457 of every member"""
        out = np.zeros(len(self.members))
        self._check(self._L.wafer_batch_norm2(self._h, _dp(out)))
        return [float(x) for x in out]

    # -- w_store, per member ---------------------------------------------------------------
    def load_state(self, i: int, idx: int, state: np.ndarray) -> None:
        i = self._member(i)
        if state.shape != self.members[i].padded_shape:
            raise ValueError("member %d: state has shape %s, not the padded shape %s" % (i, state.shape, self.members[i].padded_shape))
        self._check(self._L.wafer_batch_load_state(self._h, i, idx, _dp(state)))

    def download_state(self, i: int, idx: int) -> np.ndarray:
        i = self._member(i)
        out = np.zeros(self.members[i].padded_shape)
        self._check(self._L.wafer_batch_download_state(self._h, i, idx, _dp(out)))
        return out

    def push_state(self, active=None) -> None:
        a = self._mask(active)
        self._check(self._L.wafer_batch_push_state(self._h, self._u8(a)))

    def num_states(self) -> list:
        n = (C.c_uint32 * len(self.members))()
        self._check(self._L.wafer_batch_num_states(self._h, n))
        return [int(x) for x in n]

    def clear_states(self, active=None) -> None:
        a = self._mask(active)
        self._check(self._L.wafer_batch_clear_states(self._h, self._u8(a)))

    def clone_state_to_phi(self, idx: int, active=None) -> None:
        a = self._mask(active)
        self._check(self._L.wafer_batch_clone_state_to_phi(self._h, self._u8(a), idx))

    # -- Rayleigh-Ritz on the stores (include/wafer_hip.h) ------------------------------------------------
    def _ks(self, k, a, lo, hi, outside, default=None, max_states=False) -> list:
        """one k per member from an int (every listed member's), a sequence with one entry per member, or None (`default` for everyone;
        None: each member's own state count).  The listed entries are checked against lo .. hi (hi None: no upper bound; `outside` ends
        the message) and, with max_states, against the member's max_states.  Entries of members not listed become 0: the library does
        not read them."""
        B = len(self.members)
        if k is None:
            ks = self.num_states() if default is None else [default] * B
        else:
            ks = [int(k)] * B if np.ndim(k) == 0 else [0 if x is None else int(x) for x in k]
        if len(ks) != B:
            raise ValueError("k must hold one entry per member")
        for m in range(B):
            if a is not None and not a[m]:
                ks[m] = 0
                continue
            if ks[m] < lo or (hi is not None and ks[m] > hi):
                raise ValueError("member %d: k = %d%s" % (m, ks[m], outside))
            if max_states and ks[m] > self.members[m].max_states:
                raise ValueError("member %d: k = %d is above its max_states = %d" % (m, ks[m], self.members[m].max_states))
        return ks

    def _ritz_ks(self, k, a) -> list:
        """k of the Rayleigh-Ritz calls: 1 .. RITZ_MAX and the member's max_states"""
        return self._ks(k, a, 1, RITZ_MAX, " is outside 1 .. RITZ_MAX = %d" % RITZ_MAX, max_states=True)

    def ritz_matrices(self, k=None, active=None) -> list:
        """Context.ritz_matrices(k[m]) for every listed member (active[m] != 0; None: all) in one sums launch, one reduce and one
        read-back: per member (h, s), (k, k) each, bit for bit what a Context with its Params, potential and states gives; None for
        the members not listed.  k: an int for every listed member, one entry per member, or None for each member's state count."""
        a = self._mask(active)
        ks = self._ritz_ks(k, a)
        B = len(self.members)
        h, s = np.zeros((B, RITZ_MAX * RITZ_MAX)), np.zeros((B, RITZ_MAX * RITZ_MAX))
        self._check(self._L.wafer_batch_ritz_matrices(self._h, self._u8(a), (C.c_uint32 * B)(*ks), _dp(h), _dp(s)))
        return [None if ks[m] == 0 else (h[m, :ks[m] ** 2].reshape(ks[m], ks[m]).copy(), s[m, :ks[m] ** 2].reshape(ks[m], ks[m]).copy())
                for m in range(B)]

    def rotate_states(self, coefs, active=None) -> None:
        """Context.rotate_states(coefs[m]) for every listed member in ONE launch: l'_a = sum_j coefs[m][j, a] l_j over member m's first
        k = len(coefs[m]) stored states, in place.  coefs: one (k, k) array per member, None for members not listed."""
        a = self._mask(active)
        B = len(self.members)
        if len(coefs) != B:
            raise ValueError("coefs must hold one entry per member")
        ks, packed = [0] * B, np.zeros((B, RITZ_MAX * RITZ_MAX))
        for m in range(B):
            if a is not None and not a[m]:
                continue
            if coefs[m] is None:
                raise ValueError("member %d: is listed but has no coef (shape (k, k))" % m)
            c = np.ascontiguousarray(coefs[m], dtype=np.float64)
            if c.ndim != 2 or c.shape[0] != c.shape[1]:
                raise ValueError("member %d: coef must have shape (k, k), not %s" % (m, c.shape))
            ks[m] = c.shape[0]
            if 1 <= ks[m] <= RITZ_MAX:
                packed[m, :ks[m] ** 2] = c.ravel()
        ks = self._ritz_ks(ks, a)
        self._check(self._L.wafer_batch_rotate_states(self._h, self._u8(a), (C.c_uint32 * B)(*ks), _dp(packed)))

    def ritz(self, k=None, active=None) -> list:
        """matrices, solve, rotate for every listed member: 3 launches and one read-back whatever the members and shapes.  Per member
        {"evals": (k,), "coef": (k, k), "h": (k, k), "s": (k, k), "status": int} (h, s before the rotation), None for members not
        listed.  A member whose solve fails (linearly dependent states) has status WAFER_ERR_STATE, evals and coef None, and keeps
        its store; the others are rotated."""
        a = self._mask(active)
        ks = self._ritz_ks(k, a)
        B, KK = len(self.members), RITZ_MAX * RITZ_MAX
        evals, coef, h, s = np.zeros((B, RITZ_MAX)), np.zeros((B, KK)), np.zeros((B, KK)), np.zeros((B, KK))
        st = (C.c_int * B)()
        self._check(self._L.wafer_batch_ritz(self._h, self._u8(a), (C.c_uint32 * B)(*ks), _dp(evals), _dp(coef), _dp(h), _dp(s), st))
        out = []
        for m in range(B):
            n = ks[m]
            if n == 0:
                out.append(None)
                continue
            ok = st[m] == WAFER_OK
            out.append(dict(evals=evals[m, :n].copy() if ok else None, coef=coef[m, :n * n].reshape(n, n).copy() if ok else None,
                            h=h[m, :n * n].reshape(n, n).copy(), s=s[m, :n * n].reshape(n, n).copy(), status=int(st[m])))
        return out

    def moments(self, k=None, active=None) -> list:
        """Context.moments(k[m]) for every listed member (active[m] != 0; None: all) in one sums launch, one reduce and one read-back:
        per member {"s", "x", "y", "z", "r2", "origin"}, bit for bit what a Context with its Params and states gives, each member from
        its own centres; None for the members not listed.  k: as Batch.ritz_matrices."""
        a = self._mask(active)
        ks = self._ritz_ks(k, a)
        B, KK = len(self.members), RITZ_MAX * RITZ_MAX
        m = np.zeros((B, MOMENT_COUNT, KK))
        self._check(self._L.wafer_batch_moment_matrices(self._h, self._u8(a), (C.c_uint32 * B)(*ks), _dp(m)))
        out = []
        for mb in range(B):
            n = ks[mb]
            if n == 0:
                out.append(None)
                continue
            d = {name: m[mb, q, :n * n].reshape(n, n).copy() for q, name in enumerate(MOMENT_NAMES)}
            d["origin"] = moment_origin(self.members[mb].nx, self.members[mb].ny, self.members[mb].nz)
            out.append(d)
        return out

    def moment_counts(self) -> tuple:
        """(launches, read-backs) of moments since creation: 2 and 1 per call"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_moment_counts(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def ritz_counts(self) -> tuple:
        """(launches, read-backs) of ritz_matrices, rotate_states and ritz since creation: 2 and 1, 1 and 0, 3 and 1 per call"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_ritz_counts(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    # -- stepping the stores: subspace iteration (include/wafer_hip.h) ------------------------------------
    def _store_ks(self, k, a) -> list:
        """k of the calls that step the stores: as _ritz_ks takes it, but 0 is allowed (the member costs nothing)"""
        return self._ks(k, a, 0, None, " is negative")

    def evolve_states(self, steps: int, k=None, active=None) -> None:
        """Context.evolve_states(k[m], steps) for every listed member (active[m] != 0; None: all) in ONE launch per step, whatever the
        members and shapes (plus one batched copy where `steps` is odd: store_counts()).  k: an int for every listed member, one
        entry per member, or None for each member's state count.  phi, the other states and the members not listed keep every bit."""
        a = self._mask(active)
        ks = self._store_ks(k, a)
        self._check(self._L.wafer_batch_evolve_states(self._h, self._u8(a), (C.c_uint32 * len(ks))(*ks), int(steps)))

    def seed_states(self, k: int, seed: int, active=None) -> None:
        """k fresh stored states on every listed member: the Gaussian initial condition with seed + j, pushed, for j = 0 .. k-1 (every
        listed member gets the same seeds).  OVERWRITES phi of the listed members; the stores are not cleared first."""
        a = self._mask(active)
        B = len(self.members)
        for j in range(int(k)):
            self.set_initial_conditions(["Gaussian"] * B, [int(seed) + j] * B, active=a)
            self.push_state(active=a)

    def store_dispatch(self) -> dict:
        """what evolve_states launches: kernel, states_per_workgroup, shapes"""
        buf = C.create_string_buffer(512)
        self._check(self._L.wafer_batch_diag_store_step(self._h, buf, len(buf)))
        d = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        for key in ("states_per_workgroup", "shapes"):
            d[key] = int(d[key])
        return d

    def store_counts(self) -> int:
        """launches of evolve_states since creation: `steps` per call, plus one where `steps` is odd"""
        n = C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_store_counts(self._h, C.byref(n)))
        return n.value

    def filter_states(self, degree: int, a, b, a0, k=None, active=None) -> None:
        """Context.filter_states(k[m], degree, a[m], b[m], a0[m]) for every listed member (active[m] != 0; None: all) in ONE launch per
        recurrence step, whatever the members and shapes (plus one batched copy where `degree` is odd: filter_counts()).  a, b, a0: one
        entry per member, or a number for everyone.  phi, the other states and the members not listed keep every bit."""
        act = self._mask(active)
        ks = self._store_ks(k, act)
        B = len(self.members)
        iv = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (B,))) for x in (a, b, a0)]
        self._check(self._L.wafer_batch_filter_states(self._h, self._u8(act), (C.c_uint32 * B)(*ks), int(degree), _dp(iv[0]), _dp(iv[1]), _dp(iv[2])))

    def spectral_bound(self, active=None) -> list:
        """Context.spectral_bound() of every listed member (None for the others): one launch and one read-back"""
        act = self._mask(active)
        ub = np.full(len(self.members), np.nan)
        self._check(self._L.wafer_batch_spectral_bound(self._h, self._u8(act), _dp(ub)))
        return [float(ub[m]) if act is None or act[m] else None for m in range(len(self.members))]

    def filter_counts(self) -> tuple:
        """(launches of filter_states: `degree` per call, plus one where it is odd; launches of spectral_bound) since creation"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_filter_counts(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def _solver_calls(self, ks):
        """(mask, ritz, residuals) of solve_block and solve_filtered: the active array of a `going` list, and the loops' two callables
        on the members' first ks[m] states"""
        B = len(self.members)

        def mask(going):
            m = np.zeros(B, dtype=np.uint8)
            m[going] = 1
            return m

        def ritz(going):
            r = self.ritz(ks, active=mask(going))
            return {m: (r[m]["status"], r[m]["evals"]) for m in going}

        def residuals(going, theta):
            r = self.residuals(ks, theta=[theta.get(m) for m in range(B)], active=mask(going))
            return {m: r[m]["rho"] for m in going}

        return mask, ritz, residuals

    def solve_filtered(self, k, tolerance: float, degree: int, max_blocks: int, guard: int = 1, active=None) -> list:
        """Context.solve_filtered for every listed member at once (filtered_solve_loop): per block one filter_states, one ritz and one
        residuals call over the members still going, each with its own interval; a member whose first k - guard states have
        rho < tolerance leaves the active set and stays as it is.  -> per member the dict of Context.solve_filtered, None for members
        not listed (or with k 0)."""
        ks = self._store_ks(k, self._mask(active))
        B = len(self.members)
        mask, ritz, residuals = self._solver_calls(ks)

        def bound(going):
            ub = self.spectral_bound(active=mask(going))
            return {m: ub[m] for m in going}

        def filt(going, n, iv):
            cols = [[iv[m][q] if m in iv else 0.0 for m in range(B)] for q in range(3)]
            self.filter_states(n, cols[0], cols[1], cols[2], ks, active=mask(going))

        return filtered_solve_loop(bound, filt, ritz, residuals, ks, tolerance, degree, max_blocks, guard)

    def solve_block(self, k, tolerance: float, steps_per_block: int, max_blocks: int, active=None) -> list:
        """Context.solve_block for every listed member at once (block_solve_loop): per block one evolve_states, one ritz and one
        residuals call over the members still going; a member whose Ritz energies all moved by less than `tolerance` leaves the
        active set, as in Batch.solve.  -> per member the dict of Context.solve_block, None for members not listed (or with k 0)."""
        ks = self._store_ks(k, self._mask(active))
        mask, ritz, residuals = self._solver_calls(ks)
        return block_solve_loop(lambda going, n: self.evolve_states(n, ks, active=mask(going)), ritz, residuals, ks, tolerance, steps_per_block,
                                max_blocks)

    # -- residuals of the stores and of phi (include/wafer_hip.h) ----------------------------------------
    def residuals(self, k=None, theta=None, active=None, source: str = "states") -> list:
        """Context.residuals(k[m], theta[m], source) for every listed member (active[m] != 0; None: all): per pass one sums launch, one
        reduce and one read-back whatever the members and shapes (residual_counts()).  Per member {"theta", "r2", "norm2", "rho":
        (k,) each, "status": int}, bit for bit what a Context with its Params, potential and source gives; None for the members not
        listed.  k: as Batch.ritz (source="phi": 1).  theta: one sequence of k[m] values per member (None for members not listed), or
        None for Rayleigh quotients; there a member with a zero or non-finite state has status WAFER_ERR_STATE and None for the rest."""
        if source not in RESIDUAL_SOURCES:
            raise ValueError("source must be 'states' or 'phi', not %r" % (source,))
        a = self._mask(active)
        B = len(self.members)
        ks = self._ks(k, a, 1, 1, ": the phi source is one array (k = 1)", default=1) if source == "phi" else self._ritz_ks(k, a)
        tin = None
        if theta is not None:
            if len(theta) != B:
                raise ValueError("theta must hold one entry per member")
            tin = np.zeros((B, RITZ_MAX))
            for m in range(B):
                if ks[m] == 0:
                    continue
                if theta[m] is None:
                    raise ValueError("member %d: is listed but has no theta" % m)
                t = np.atleast_1d(np.asarray(theta[m], dtype=np.float64))
                if t.shape != (ks[m],):
                    raise ValueError("member %d: theta must hold k = %d values, not shape %s" % (m, ks[m], t.shape))
                if not np.all(np.isfinite(t)):
                    raise ValueError("member %d: theta must be finite" % m)
                tin[m, :ks[m]] = t
        th, r2, s = np.zeros((B, RITZ_MAX)), np.zeros((B, RITZ_MAX)), np.zeros((B, RITZ_MAX))
        st = (C.c_int * B)()
        self._check(self._L.wafer_batch_residuals(self._h, RESIDUAL_SOURCES[source], self._u8(a), (C.c_uint32 * B)(*ks),
                                                  None if tin is None else _dp(tin), _dp(th), _dp(r2), _dp(s), st))
        out = []
        for m in range(B):
            n = ks[m]
            if n == 0:
                out.append(None)
            elif st[m] != WAFER_OK:
                out.append(dict(theta=None, r2=None, norm2=None, rho=None, status=int(st[m])))
            else:
                out.append(dict(theta=th[m, :n].copy(), r2=r2[m, :n].copy(), norm2=s[m, :n].copy(), rho=np.sqrt(r2[m, :n] / s[m, :n]),
                                status=int(st[m])))
        return out

    def residual_counts(self) -> tuple:
        """(launches, read-backs) of residuals since creation: 2 and 1 per call with theta given, 4 and 2 per Rayleigh-mode call"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_residual_counts(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def observables(self) -> list:
        """compute_observables (un-normalised) of every member"""
        o = (_Obs * len(self.members))()
        self._check(self._L.wafer_batch_observables(self._h, o))
        return [dict(energy=x.energy, norm2=x.norm2, v_infinity=x.v_infinity, r2=x.r2) for x in o]

    def normalise(self, norm2s, active=None) -> None:
        n2 = np.ascontiguousarray(np.asarray(norm2s, dtype=np.float64))
        if n2.shape != (len(self.members),):
            raise ValueError("norm2s must hold one value per member")
        a = self._mask(active)
        self._check(self._L.wafer_batch_normalise(self._h, self._u8(a), _dp(n2)))

    def solve(self, tolerance: float, screen_update: int, max_steps=None, max_records: int | None = None) -> list:
        """-> per member (rows, final, converged, status) in Context.solve_state's format; status is WAFER_OK,
        WAFER_ERR_MAX_STEP or WAFER_ERR_STATE.  max_records (rows kept per member; None: every row a run bounded by max_steps
        can produce, else 100000 shared out over the members, at least 1000 each).  Pushes no state."""
        return self._solve(None, tolerance, screen_update, max_steps, max_records)

    def solve_state(self, wnum: int, tolerance: float, screen_update: int, max_steps=None, max_records: int | None = None) -> list:
        """solve() for state `wnum`, each member against its own first `wnum` stored states; a member that converges has its phi
        pushed to its store.  A member whose store holds fewer than `wnum` states gets the status WAFER_ERR_STATE and is left
        as it is."""
        return self._solve(self._wnum(wnum), tolerance, screen_update, max_steps, max_records)

    def _solve(self, wnum, tolerance, screen_update, max_steps, max_records) -> list:
        B = len(self.members)
        if max_records is None:
            if max_steps is not None:   # rows at steps 0, su, 2 su, ... up to the first step past max_steps
                max_records = int(max_steps) // max(1, int(screen_update)) + 2
            else:
                max_records = max(1000, 100000 // max(1, B))
        recs = (_Record * (B * max_records))()
        n = (C.c_size_t * B)()
        fin = (_ObsOut * B)()
        st = (C.c_int * B)()
        tail = (tolerance, screen_update, 0 if max_steps is None else 1, 0 if max_steps is None else int(max_steps), recs,
                max_records, n, fin, st)
        if wnum is None:
            self._check(self._L.wafer_batch_solve(self._h, *tail))
        else:
            self._check(self._L.wafer_batch_solve_state(self._h, wnum, *tail))
        out = []
        for m in range(B):
            rows = []
            for k in range(min(n[m], max_records)):
                r = recs[m * max_records + k]
                rows.append(dict(step=r.step, tau=r.tau, energy=r.obs.energy, norm2=r.obs.norm2,
                                 v_infinity=r.obs.v_infinity, r2=r.obs.r2, diff=r.diff))
            f = fin[m]
            final = dict(state=f.state, energy=f.energy, binding_energy=f.binding_energy, r=f.r, l_r=f.l_r)
            out.append((rows, final, st[m] == WAFER_OK, st[m]))
        return out

    def last_evolve_ms(self):
        ms, steps = C.c_float(0.0), C.c_uint64(0)
        self._check(self._L.wafer_batch_last_evolve_ms(self._h, C.byref(ms), C.byref(steps)))
        return ms.value, steps.value

    def kernel_name(self) -> str:
        return self._L.wafer_batch_kernel_name(self._h).decode()

    def steps_per_launch(self) -> int:
        """K of the pass a ground-state evolve of at least K steps launches; 1: the one-step kernel"""
        k = self._L.wafer_batch_steps_per_launch(self._h)
        if k < 1:
            self._check(k)
        return k

    def set_step_variant(self, variant: int) -> None:
        """-1: default dispatch, 0: one step per launch, 1: fused passes wherever an instantiation exists (the same bits)"""
        self._check(self._L.wafer_batch_set_step_variant(self._h, int(variant)))

    def dispatch(self) -> dict:
        """what a ground-state evolve would launch: stencil, kernel, steps_per_pass, tile, lds_bytes, remainder, variant, dtype,
        and, on a batch of several shapes, shapes (their number, as the line gives it)"""
        buf = C.create_string_buffer(512)
        self._check(self._L.wafer_batch_diag_dispatch(self._h, buf, len(buf)))
        d = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        for k in ("steps_per_pass", "lds_bytes", "variant"):
            d[k] = int(d[k])
        return d

    def passes(self) -> tuple:
        """(fused passes, one-step launches) since creation"""
        f, s = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_passes(self._h, C.byref(f), C.byref(s)))
        return f.value, s.value

    def set_gs_variant(self, variant: int) -> None:
        """the form of excited steps and orthogonalise: -1 default dispatch (sequential), 0 sequential, 1 one pass (wnum <= 4)"""
        self._check(self._L.wafer_batch_set_gs_variant(self._h, int(variant)))

    def gs_dispatch(self, wnum: int) -> dict:
        """what an excited step with `wnum` would launch: wnum, form, launches_per_step, kernels, variant, dtype, onepass_bytes and,
        on a batch of several shapes with state stores, shapes (their number)"""
        buf = C.create_string_buffer(768)
        self._check(self._L.wafer_batch_diag_gs(self._h, int(wnum), buf, len(buf)))
        d = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        for k in ("wnum", "launches_per_step", "variant", "onepass_bytes", "shapes"):
            if k in d:
                d[k] = int(d[k])
        return d

    def gs_steps(self) -> tuple:
        """(one-pass, sequential) excited steps and orthogonalise calls since creation"""
        o, s = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.wafer_batch_diag_gs_steps(self._h, C.byref(o), C.byref(s)))
        return o.value, s.value
