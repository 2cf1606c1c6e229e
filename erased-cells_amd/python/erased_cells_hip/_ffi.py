"""ctypes binding of liberased_cells_hip.so (include/erased_cells.h).

There is no fallback: if the shared library is missing or a symbol is absent the
import fails loudly, and every compute call raises unless a HIP device is bound.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
AMD_DIR = os.path.dirname(os.path.dirname(_PKG))          # erased-cells_amd/
REPO = os.path.dirname(AMD_DIR)
SO_PATH = os.environ.get("EC_HIP_LIB") or os.path.join(AMD_DIR, "liberased_cells_hip.so")  # EC_HIP_LIB: A/B builds
CSRC = os.path.join(AMD_DIR, "csrc")

EC_OK, EC_ERR_NARROWING, EC_ERR_UNSUPPORTED_TYPE, EC_ERR_LENGTH, EC_ERR_HIP, EC_ERR_RCCL, EC_ERR_ARG, \
    EC_ERR_NOT_INITIALIZED = range(8)
EC_RESAMPLE_NEAREST, EC_RESAMPLE_BILINEAR, EC_RESAMPLE_AVERAGE = 0, 1, 5  # ec_resample: GDAL's GRIORA_* numbers
EC_WINDOW_MAX_REDUCTION = 64
# ec_cmp: a relation is the truth table over Ordering — bit 0 Less, bit 1 Equal, bit 2 Greater
EC_CMP_LT, EC_CMP_EQ, EC_CMP_LE, EC_CMP_GT, EC_CMP_NE, EC_CMP_GE = 1, 2, 3, 4, 5, 6
EC_CAST_AS, EC_CAST_ROUND = 0, 1  # ec_cast_mode: Rust's `as` / the storing rule (clamp, round half away from zero)
EC_FOCAL_SUM, EC_FOCAL_MEAN, EC_FOCAL_MIN, EC_FOCAL_MAX = range(4)  # ec_focal_op
EC_FOCAL_RADIUS_CAP = 7
EC_FOCAL_WHOLE, EC_FOCAL_NORMALIZE = 1, 2  # flags of ec_focal / ec_focal_convolve
EC_FOCAL_RANK_MAX_TAPS = 64  # the footprint of ec_focal_rank / ec_focal_majority
EC_COMPOSITE_FIRST, EC_COMPOSITE_LAST, EC_COMPOSITE_MIN, EC_COMPOSITE_MAX, EC_COMPOSITE_SUM, EC_COMPOSITE_MEAN = range(6)  # ec_composite_op
EC_COMPOSITE_MAX_LAYERS, EC_COMPOSITE_NONE = 64, 255
EC_RANK_LOWER, EC_RANK_UPPER = range(2)  # ec_rank_method
EC_RANK_MAX_DEN = 65535
EC_ZONAL_MAX_ZONES = 256
EC_ZONAL_TABLE_MAX_ZONES = 1 << 24
EC_RECLASS_MAX_BREAKS, EC_RECLASS_TABLE_BYTES = 255, 4384
EC_RECLASS_HAS_NODATA, EC_RECLASS_DROPS = 1, 2  # ec_reclass_table.flags
EC_DISTANCE_MAX_SIDE, EC_DISTANCE_UNLIMITED = 32768, 0xFFFFFFFF  # ec_distance: the longest side, max_sq of "no limit"
EC_REGIONS_MAX_SIDE = 32768  # ec_regions: the longest side
EC_REGIONS_ROOT, EC_REGIONS_DENSE = range(2)  # ec_regions_numbering


class _Payload(C.Union):
    _fields_ = [("u8", C.c_uint8), ("u16", C.c_uint16), ("u32", C.c_uint32), ("u64", C.c_uint64),
                ("i8", C.c_int8), ("i16", C.c_int16), ("i32", C.c_int32), ("i64", C.c_int64),
                ("f32", C.c_float), ("f64", C.c_double), ("bits", C.c_uint64)]


class EcValue(C.Structure):
    """ec_value: 16-byte tagged scalar (CellValue, src/value.rs:12-20)."""
    _fields_ = [("dtype", C.c_uint8), ("pad_", C.c_uint8 * 7), ("v", _Payload)]


class EcExprStep(C.Structure):
    """ec_expr_step: reg[dst] = a op b (include/erased_cells.h)."""
    _fields_ = [("op", C.c_int8), ("a", C.c_int8), ("b", C.c_int8), ("dst", C.c_int8)]


class _MomentsInt(C.Structure):
    _fields_ = [("sum", C.c_int64), ("sq_lo", C.c_uint64), ("sq_hi", C.c_uint64)]


class _MomentsF64(C.Structure):
    _fields_ = [("pivot", C.c_double), ("s1", C.c_double), ("s2", C.c_double)]


class _MomentsUnion(C.Union):
    _fields_ = [("i", _MomentsInt), ("f", _MomentsF64)]


class EcMoments(C.Structure):
    """ec_moments: the 64-byte record one ec_stats_device launch leaves on the device (include/erased_cells.h)."""
    _fields_ = [("count", C.c_uint64), ("keys2", C.c_int64 * 2), ("kind", C.c_int32), ("dtype", C.c_int32),
                ("u", _MomentsUnion), ("reserved", C.c_uint64)]


class EcStats(C.Structure):
    """ec_stats: what ec_stats_fold makes of one or several records."""
    _fields_ = [("count", C.c_uint64), ("min", EcValue), ("max", EcValue), ("sum", C.c_double), ("mean", C.c_double),
                ("stddev", C.c_double)]


class EcReclassTable(C.Structure):
    """ec_reclass_table: what ec_reclass_table_build writes and ec_reclass reads on the device (include/erased_cells.h)."""
    _fields_ = [("t", C.c_int32), ("dt", C.c_int32), ("n_breaks", C.c_int32), ("n_reached", C.c_int32), ("flags", C.c_uint32),
                ("reserved0", C.c_uint32), ("nodata_bits", C.c_uint64), ("reserved1", C.c_uint64), ("thr", C.c_int64 * 255),
                ("value_bits", C.c_uint64 * 256), ("valid", C.c_uint8 * 256)]


VP, SZ, I32, U8P = C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p
PV = C.POINTER(EcValue)
PVP, PSZ = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)


class EcCommUid(C.Structure):
    """ec_comm_uid (ncclUniqueId): 128 opaque bytes rank 0 hands to the other ranks."""
    _fields_ = [("bytes", C.c_char * 128)]


# ec_shard_fn: ec_status fn(int32 shard, int32 device, ec_stream stream, void* user)
SHARD_FN = C.CFUNCTYPE(C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p)

# name -> (restype, argtypes): every symbol include/erased_cells.h declares.
SIGNATURES = {
    "ec_union": (C.c_uint8, [C.c_uint8, C.c_uint8]),
    "ec_can_fit_into": (I32, [C.c_uint8, C.c_uint8]),
    "ec_size_of": (SZ, [C.c_uint8]),
    "ec_neg_result_type": (C.c_uint8, [C.c_uint8]),
    "ec_min_value": (I32, [C.c_uint8, PV]),
    "ec_max_value": (I32, [C.c_uint8, PV]),
    "ec_nodata_default": (I32, [C.c_uint8, PV]),
    "ec_value_convert": (I32, [PV, C.c_uint8, PV]),
    "ec_value_to_f64": (C.c_double, [PV]),
    "ec_shard_range": (I32, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ec_abi_version": (I32, []),
    "ec_init": (I32, [I32]),
    "ec_set_device": (I32, [I32]),
    "ec_get_device": (I32, [C.POINTER(I32)]),
    "ec_shutdown": (I32, []),
    "ec_last_error_string": (C.c_char_p, []),
    "ec_last_narrowing": (I32, [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "ec_device_info": (I32, [C.POINTER(I32), C.POINTER(C.c_uint64), C.c_char_p, SZ]),
    "ec_alloc": (I32, [C.POINTER(VP), SZ]),
    "ec_free": (I32, [VP]),
    "ec_alloc_async": (I32, [C.POINTER(VP), SZ, VP]),
    "ec_free_async": (I32, [VP, VP]),
    "ec_free_ordered": (I32, [VP, VP, VP]),
    "ec_pool_trim": (I32, [SZ]),
    "ec_upload": (I32, [VP, VP, SZ, VP]),
    "ec_download": (I32, [VP, VP, SZ, VP]),
    "ec_copy": (I32, [VP, VP, SZ, VP]),
    "ec_stream_create": (I32, [C.POINTER(VP)]),
    "ec_prepare_stream": (I32, [VP]),
    "ec_release_stream": (I32, [VP]),
    "ec_stream_destroy": (I32, [VP]),
    "ec_stream_sync": (I32, [VP]),
    "ec_binop": (I32, [I32, C.c_uint8, VP, C.c_uint8, VP, SZ, VP, VP]),
    "ec_binop_scalar": (I32, [I32, C.c_uint8, VP, SZ, PV, VP, VP]),
    "ec_masked_binop": (I32, [I32, C.c_uint8, VP, U8P, C.c_uint8, VP, U8P, SZ, VP, U8P, VP]),
    "ec_fused": (I32, [I32, I32, I32, C.POINTER(C.c_uint8), C.POINTER(VP), PV, SZ, VP, VP]),
    "ec_masked_fused": (I32, [I32, I32, I32, C.POINTER(C.c_uint8), C.POINTER(VP), C.POINTER(VP), PV, SZ, VP, U8P, VP]),
    "ec_expr": (I32, [C.POINTER(C.c_uint8), C.POINTER(VP), I32, PV, I32, C.POINTER(EcExprStep), I32, SZ, VP, VP]),
    "ec_expr_min_max": (I32, [C.POINTER(C.c_uint8), C.POINTER(VP), C.POINTER(VP), I32, PV, I32, C.POINTER(EcExprStep), I32, SZ, PV, PV, VP]),
    "ec_expr_min_max_keys": (I32, [C.POINTER(C.c_uint8), C.POINTER(VP), C.POINTER(VP), I32, PV, I32, C.POINTER(EcExprStep), I32, SZ, VP, VP]),
    "ec_sharded_expr_min_max": (I32, [VP, C.POINTER(C.c_uint8), C.POINTER(PVP), C.POINTER(PVP), I32, PV, I32, C.POINTER(EcExprStep), I32, PSZ, PV, PV]),
    "ec_expr_source": (I32, [C.POINTER(C.c_uint8), I32, I32, C.POINTER(EcExprStep), I32, C.c_char_p, C.c_char_p, SZ, C.POINTER(SZ)]),
    "ec_host_alloc": (I32, [PVP, SZ]),
    "ec_host_free": (I32, [VP]),
    "ec_host_masked_expr": (I32, [C.POINTER(C.c_uint8), C.POINTER(VP), C.POINTER(PV), I32, PV, I32, C.POINTER(EcExprStep), I32, SZ, VP,
                                  C.POINTER(C.c_double), VP, SZ]),
    "ec_host_expr": (I32, [C.POINTER(C.c_uint8), C.POINTER(VP), I32, PV, I32, C.POINTER(EcExprStep), I32, SZ, VP, SZ]),
    "ec_masked_expr": (I32, [C.POINTER(C.c_uint8), C.POINTER(VP), C.POINTER(VP), I32, PV, I32, C.POINTER(EcExprStep), I32, SZ, VP, U8P, VP]),
    "ec_neg": (I32, [C.c_uint8, VP, SZ, VP, VP]),
    "ec_convert": (I32, [C.c_uint8, VP, C.c_uint8, VP, SZ, VP]),
    "ec_fill": (I32, [C.c_uint8, VP, SZ, PV, VP]),
    "ec_min_max": (I32, [C.c_uint8, VP, U8P, SZ, PV, PV, VP]),
    "ec_min_max_keys": (I32, [C.c_uint8, VP, U8P, SZ, VP, VP]),
    "ec_min_max_decode": (I32, [C.c_uint8, C.POINTER(C.c_int64), PV, PV]),
    "ec_allreduce_min_max_keys": (I32, [VP, VP, VP]),
    "ec_allreduce_counts": (I32, [VP, VP, VP]),
    "ec_comm_get_unique_id": (I32, [C.POINTER(EcCommUid)]),
    "ec_comm_init_rank": (I32, [C.POINTER(EcCommUid), I32, I32, PVP]),
    "ec_comm_init_all": (I32, [C.POINTER(I32), I32, PVP]),
    "ec_comm_destroy": (I32, [VP]),
    "ec_shard_group_create": (I32, [C.POINTER(I32), I32, C.c_uint32, PVP]),
    "ec_shard_group_destroy": (I32, [VP]),
    "ec_shard_group_size": (I32, [VP]),
    "ec_shard_group_shard": (I32, [VP, I32, C.POINTER(I32), PVP]),
    "ec_shard_group_foreach": (I32, [VP, SHARD_FN, VP]),
    "ec_shard_group_sync": (I32, [VP]),
    "ec_shard_group_stat": (I32, [VP, C.c_char_p, C.POINTER(C.c_int64)]),
    "ec_sharded_alloc": (I32, [VP, PSZ, PVP]),
    "ec_sharded_free": (I32, [VP, PVP]),
    "ec_sharded_upload": (I32, [VP, PVP, VP, PSZ, PSZ]),
    "ec_sharded_download": (I32, [VP, VP, PVP, PSZ, PSZ]),
    "ec_sharded_binop": (I32, [VP, I32, C.c_uint8, PVP, C.c_uint8, PVP, PSZ, PVP]),
    "ec_sharded_masked_binop": (I32, [VP, I32, C.c_uint8, PVP, PVP, C.c_uint8, PVP, PVP, PSZ, PVP, PVP]),
    "ec_sharded_convert": (I32, [VP, C.c_uint8, PVP, C.c_uint8, PVP, PSZ]),
    "ec_sharded_mask_from_nodata": (I32, [VP, C.c_uint8, PVP, PSZ, PV, PVP]),
    "ec_sharded_host_expr": (I32, [VP, C.POINTER(C.c_uint8), C.POINTER(VP), C.POINTER(PV), I32, PV, I32, C.POINTER(EcExprStep), I32, C.c_uint64,
                                   C.c_uint64, VP, C.POINTER(C.c_double), VP, SZ]),
    "ec_sharded_expr": (I32, [VP, C.POINTER(C.c_uint8), C.POINTER(PVP), C.POINTER(PVP), I32, PV, I32, C.POINTER(EcExprStep), I32, PSZ, PVP, PVP]),
    "ec_sharded_fused": (I32, [VP, I32, I32, I32, C.POINTER(C.c_uint8), C.POINTER(PVP), C.POINTER(PVP), PV, PSZ, PVP, PVP]),
    "ec_sharded_min_max": (I32, [VP, C.c_uint8, PVP, PVP, PSZ, PV, PV]),
    "ec_sharded_counts": (I32, [VP, PVP, PSZ, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ec_buffer_cmp": (I32, [C.c_uint8, VP, SZ, C.c_uint8, VP, SZ, C.POINTER(I32), VP]),
    "ec_first_difference": (I32, [C.c_uint8, VP, VP, SZ, C.POINTER(C.c_uint64), VP]),
    "ec_mask_from_nodata": (I32, [C.c_uint8, VP, SZ, PV, U8P, VP]),
    "ec_mask_select": (I32, [C.c_uint8, VP, U8P, SZ, PV, VP, VP]),
    "ec_mask_and": (I32, [U8P, U8P, SZ, U8P, VP]),
    "ec_mask_or": (I32, [U8P, U8P, SZ, U8P, VP]),
    "ec_mask_not": (I32, [U8P, SZ, U8P, VP]),
    "ec_mask_counts": (I32, [U8P, SZ, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), VP]),
    "ec_mask_counts_device": (I32, [U8P, SZ, VP, VP]),
    "ec_compare": (I32, [I32, C.c_uint8, VP, U8P, C.c_uint8, VP, U8P, SZ, U8P, VP]),
    "ec_compare_scalar": (I32, [I32, C.c_uint8, VP, U8P, SZ, PV, U8P, VP]),
    "ec_select": (I32, [C.c_uint8, VP, VP, U8P, SZ, VP, VP]),
    "ec_masked_select": (I32, [C.c_uint8, VP, U8P, VP, U8P, U8P, SZ, VP, U8P, VP]),
    "ec_sharded_compare": (I32, [VP, I32, C.c_uint8, PVP, PVP, C.c_uint8, PVP, PVP, PSZ, PVP]),
    "ec_sharded_compare_scalar": (I32, [VP, I32, C.c_uint8, PVP, PVP, PSZ, PV, PVP]),
    "ec_cast": (I32, [I32, C.c_uint8, VP, C.c_uint8, VP, SZ, VP]),
    "ec_cast_scaled": (I32, [C.c_uint8, VP, U8P, SZ, C.c_double, C.c_double, C.c_uint8, PV, VP, VP]),
    "ec_sharded_cast": (I32, [VP, I32, C.c_uint8, PVP, C.c_uint8, PVP, PSZ]),
    "ec_sharded_cast_scaled": (I32, [VP, C.c_uint8, PVP, PVP, PSZ, C.c_double, C.c_double, C.c_uint8, PV, PVP]),
    "ec_stats_device": (I32, [C.c_uint8, VP, U8P, SZ, VP, VP]),
    "ec_stats_fold": (I32, [VP, I32, VP]),
    "ec_stats_compute": (I32, [C.c_uint8, VP, U8P, SZ, VP, VP]),
    "ec_sharded_stats": (I32, [VP, C.c_uint8, PVP, PVP, PSZ, VP]),
    "ec_window": (I32, [C.c_uint8, VP, U8P] + [C.c_uint64] * 8 + [VP, U8P, VP]),
    "ec_window_resample": (I32, [I32, C.c_uint8, VP, U8P] + [C.c_uint64] * 8 + [VP, U8P, VP]),
    "ec_window_put": (I32, [C.c_uint8, VP, U8P, C.c_uint64, C.c_uint64, VP, U8P] + [C.c_uint64] * 4 + [VP]),
    "ec_focal_result_type": (C.c_uint8, [I32, C.c_uint8]),
    "ec_focal": (I32, [I32, C.c_uint8, VP, U8P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, VP, U8P, VP]),
    "ec_focal_convolve": (I32, [C.c_uint8, VP, U8P, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.c_uint32, VP, U8P, VP]),
    "ec_focal_rank": (I32, [C.c_uint8, VP, U8P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, I32, C.c_uint32, VP, U8P, VP]),
    "ec_focal_majority": (I32, [C.c_uint8, VP, U8P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, VP, U8P, VP]),
    "ec_zonal_workspace_bytes": (SZ, [I32]),
    "ec_zonal_stats_device": (I32, [C.c_uint8, VP, U8P, C.c_uint8, VP, SZ, I32, VP, VP, VP]),
    "ec_zonal_stats_compute": (I32, [C.c_uint8, VP, U8P, C.c_uint8, VP, SZ, I32, VP, VP]),
    "ec_sharded_zonal_stats": (I32, [VP, C.c_uint8, PVP, PVP, C.c_uint8, PVP, PSZ, I32, VP]),
    "ec_zonal_broadcast": (I32, [C.c_uint8, VP, SZ, I32, C.c_uint8, VP, VP, U8P, VP]),
    "ec_zonal_table_workspace_bytes": (SZ, [C.c_uint8, I32]),
    "ec_zonal_table_device": (I32, [C.c_uint8, VP, U8P, C.c_uint8, VP, SZ, I32, VP, VP, VP]),
    "ec_zonal_table_compute": (I32, [C.c_uint8, VP, U8P, C.c_uint8, VP, SZ, I32, VP, VP]),
    "ec_sharded_zonal_table": (I32, [VP, C.c_uint8, PVP, PVP, C.c_uint8, PVP, PSZ, I32, VP]),
    "ec_zonal_lookup": (I32, [C.c_uint8, VP, SZ, I32, C.c_uint8, VP, VP, U8P, VP]),
    "ec_reclass_table_build": (I32, [C.c_uint8, C.c_uint8, VP, I32, I32, C.c_uint8, PV, U8P, PV, VP]),
    "ec_reclass": (I32, [C.c_uint8, VP, U8P, SZ, C.c_uint8, VP, VP, U8P, VP]),
    "ec_sharded_reclass": (I32, [VP, C.c_uint8, PVP, PVP, PSZ, C.c_uint8, PVP, PVP, PVP]),
    "ec_distance_workspace_bytes": (SZ, [C.c_uint64, C.c_uint64]),
    "ec_distance": (I32, [U8P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint8, VP, U8P, VP, VP]),
    "ec_regions_workspace_bytes": (SZ, [C.c_uint64, C.c_uint64]),
    "ec_regions": (I32, [C.c_uint8, VP, U8P, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_uint64, VP, U8P, VP, VP, VP]),
    "ec_composite_result_type": (C.c_uint8, [I32, C.c_uint8]),
    "ec_composite": (I32, [I32, C.c_uint8, PVP, PVP, I32, SZ, C.c_uint32, VP, U8P, U8P, VP]),
    "ec_sharded_composite": (I32, [VP, I32, C.c_uint8, C.POINTER(PVP), C.POINTER(PVP), I32, PSZ, C.c_uint32, PVP, PVP, PVP]),
    "ec_composite_rank": (I32, [C.c_uint8, PVP, PVP, I32, SZ, C.c_uint32, C.c_uint32, I32, C.c_uint32, VP, U8P, U8P, VP]),
    "ec_sharded_composite_rank": (I32, [VP, C.c_uint8, C.POINTER(PVP), C.POINTER(PVP), I32, PSZ, C.c_uint32, C.c_uint32, I32, C.c_uint32, PVP, PVP, PVP]),
    "ec_synth_fill": (I32, [C.c_uint8, VP, SZ, C.c_uint64, C.c_uint64, C.c_double, C.c_double, VP]),
    "ec_synth_mask": (I32, [U8P, SZ, C.c_uint64, C.c_uint64, C.c_uint32, VP]),
    "ec_tune_set": (I32, [C.c_char_p, C.c_int64]),
    "ec_stat_get": (I32, [C.c_char_p, C.POINTER(C.c_int64)]),
}


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, f"-j{jobs}", "-s"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean", "-s"])
    subprocess.check_call(args)
    return SO_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and loads it by a different
        # file name than this library's DT_NEEDED entry.  If torch comes second it brings up a second
        # runtime copy that cannot see the device; if torch is loaded first the dynamic loader resolves
        # our libamdhip64.so.7 to torch's copy and both share one runtime.  So: torch first, when present.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(SO_PATH):
            raise ImportError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              f"(or `make -C {CSRC}`); there is no CPU fallback")
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


class EcError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"[ec_status {status}] {message}")
        self.status = status


class NarrowingError(EcError):
    """Error::NarrowingError{src,dst} (src/error.rs:14-15)."""

    def __init__(self, message: str, src: int, dst: int):
        super().__init__(EC_ERR_NARROWING, message)
        self.src, self.dst = src, dst


def check(status: int) -> None:
    if status == EC_OK:
        return
    L = lib()
    msg = (L.ec_last_error_string() or b"").decode()
    if status == EC_ERR_NARROWING:
        s, d = C.c_uint8(), C.c_uint8()
        L.ec_last_narrowing(C.byref(s), C.byref(d))
        raise NarrowingError(msg, s.value, d.value)
    raise EcError(status, msg)


class tuned:
    """`with ec.tuned(binop_variant=1, map_u=4): ...` — the knobs of `ec_tune_set` set for the block.  Each knob named is put back on exit
    to the value `ec_stat_get("tune.<knob>")` read on entry (blocks nest); an unknown knob or a value `ec_tune_set` refuses raises EcError
    with every knob as it was."""

    def __init__(self, **knobs: int):
        self.knobs = knobs
        self.previous: dict = {}

    def __enter__(self):
        L, v = lib(), C.c_int64()
        previous = {}
        for key in self.knobs:
            check(L.ec_stat_get(b"tune." + key.encode(), C.byref(v)))
            previous[key] = v.value
        self.previous = {}
        try:
            for key, value in self.knobs.items():
                self.previous[key] = previous[key]
                check(L.ec_tune_set(key.encode(), value))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        return False

    def _restore(self):
        for key, value in reversed(list(self.previous.items())):
            check(lib().ec_tune_set(key.encode(), value))
        self.previous = {}
