"""ctypes binding of libmpich_reduce_local.so -- the MI355X MPI_Reduce_local.

This is host plumbing for tests, the benchmark and the smoke check; the
product is the C ABI declared in include/mpi_reduce_local.h (see
INTEGRATION.md for how MPICH links it).  Constants mirror that header, which
mirrors the reference's mpi.h.in / configure.ac values.

The library is loaded from mpich-pip_amd/lib/ (built by `make -C
mpich-pip_amd` or __graft_entry__.build()).  A missing library raises
immediately: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libmpich_reduce_local.so")

# ---- error classes (mpi.h.in:784-811)
MPI_SUCCESS = 0
MPI_ERR_BUFFER = 1
MPI_ERR_COUNT = 2
MPI_ERR_TYPE = 3
MPI_ERR_OP = 9
MPI_ERR_ARG = 12
MPI_ERR_OTHER = 15

MPI_ERRORS_ARE_FATAL = 0x54000000
MPI_ERRORS_RETURN = 0x54000001

# ---- ops (mpi.h.in:310-325)
MPI_OP_NULL = 0x18000000
MPI_MAX = 0x58000001
MPI_MIN = 0x58000002
MPI_SUM = 0x58000003
MPI_PROD = 0x58000004
MPI_LAND = 0x58000005
MPI_BAND = 0x58000006
MPI_LOR = 0x58000007
MPI_BOR = 0x58000008
MPI_LXOR = 0x58000009
MPI_BXOR = 0x5800000A
MPI_MINLOC = 0x5800000B
MPI_MAXLOC = 0x5800000C
MPI_REPLACE = 0x5800000D
MPI_NO_OP = 0x5800000E

OPS = {
    "MPI_MAX": MPI_MAX, "MPI_MIN": MPI_MIN, "MPI_SUM": MPI_SUM, "MPI_PROD": MPI_PROD,
    "MPI_LAND": MPI_LAND, "MPI_BAND": MPI_BAND, "MPI_LOR": MPI_LOR, "MPI_BOR": MPI_BOR,
    "MPI_LXOR": MPI_LXOR, "MPI_BXOR": MPI_BXOR, "MPI_MINLOC": MPI_MINLOC, "MPI_MAXLOC": MPI_MAXLOC,
}

# ---- datatypes, x86-64 values (configure.ac:3442-3705)
MPI_DATATYPE_NULL = 0x0C000000
DATATYPES = {
    "MPI_CHAR": 0x4C000101,
    "MPI_UNSIGNED_CHAR": 0x4C000102,
    "MPI_SHORT": 0x4C000203,
    "MPI_UNSIGNED_SHORT": 0x4C000204,
    "MPI_INT": 0x4C000405,
    "MPI_UNSIGNED": 0x4C000406,
    "MPI_LONG": 0x4C000807,
    "MPI_UNSIGNED_LONG": 0x4C000808,
    "MPI_LONG_LONG": 0x4C000809,
    "MPI_FLOAT": 0x4C00040A,
    "MPI_DOUBLE": 0x4C00080B,
    "MPI_LONG_DOUBLE": 0x4C00100C,
    "MPI_BYTE": 0x4C00010D,
    "MPI_WCHAR": 0x4C00040E,
    "MPI_2INT": 0x4C000816,
    "MPI_SIGNED_CHAR": 0x4C000118,
    "MPI_UNSIGNED_LONG_LONG": 0x4C000819,
    "MPI_FLOAT_INT": 0x8C000000,
    "MPI_DOUBLE_INT": 0x8C000001,
    "MPI_LONG_DOUBLE_INT": 0x8C000004,
    "MPI_LONG_INT": 0x8C000002,
    "MPI_SHORT_INT": 0x8C000003,
    "MPI_INT8_T": 0x4C000137,
    "MPI_INT16_T": 0x4C000238,
    "MPI_INT32_T": 0x4C000439,
    "MPI_INT64_T": 0x4C00083A,
    "MPI_UINT8_T": 0x4C00013B,
    "MPI_UINT16_T": 0x4C00023C,
    "MPI_UINT32_T": 0x4C00043D,
    "MPI_UINT64_T": 0x4C00083E,
    "MPI_C_BOOL": 0x4C00013F,
    "MPI_C_FLOAT_COMPLEX": 0x4C000840,
    "MPI_C_DOUBLE_COMPLEX": 0x4C001041,
    "MPI_C_LONG_DOUBLE_COMPLEX": 0x4C002042,
    "MPIX_C_FLOAT16": 0x4C000246,
    "MPI_AINT": 0x4C000843,
    "MPI_OFFSET": 0x4C000844,
    "MPI_COUNT": 0x4C000845,
}
globals().update(DATATYPES)

# Every symbol include/mpi_reduce_local.h declares (checked by the CPU tests).
EXPORTED_SYMBOLS = [
    "MPI_Reduce_local", "PMPI_Reduce_local", "MPIR_Reduce_local",
    "MPIR_MAXF", "MPIR_MINF", "MPIR_SUM", "MPIR_PROD", "MPIR_LAND", "MPIR_BAND", "MPIR_LOR",
    "MPIR_BOR", "MPIR_LXOR", "MPIR_BXOR", "MPIR_MAXLOC", "MPIR_MINLOC", "MPIR_REPLACE", "MPIR_NO_OP",
    "MPIR_MAXF_check_dtype", "MPIR_MINF_check_dtype", "MPIR_SUM_check_dtype", "MPIR_PROD_check_dtype",
    "MPIR_LAND_check_dtype", "MPIR_BAND_check_dtype", "MPIR_LOR_check_dtype", "MPIR_BOR_check_dtype",
    "MPIR_LXOR_check_dtype", "MPIR_BXOR_check_dtype", "MPIR_MAXLOC_check_dtype",
    "MPIR_MINLOC_check_dtype", "MPIR_REPLACE_check_dtype", "MPIR_NO_OP_check_dtype",
    "MPIR_Op_table", "MPIR_Op_check_dtype_table",
    "MPI_Op_create", "PMPI_Op_create", "MPI_Op_free", "PMPI_Op_free",
    "MPI_Op_commutative", "PMPI_Op_commutative", "MPIR_Op_is_commutative",
    "MPI_Error_class", "MPI_Error_string",
    "MPIX_Reduce_local_stream", "MPIX_Reduce_local_set_errhandler", "MPIX_Reduce_local_get_errhandler",
    "MPIX_Reduce_local_multi", "MPIR_Hip_combine",
    "MPIX_Reduce_local_batch", "MPIR_Hip_reduce_batch", "MPIR_Hip_batch_plan_info",
    "MPIX_Reduce_local_strided", "MPIR_Hip_reduce_strided", "MPIR_Hip_strided_plan_info",
    "MPIR_Hip_set_strided_wide_bytes", "MPIR_Hip_strided_test_max_groups",
    "MPIX_Reduce_local_subarray", "MPIR_Hip_reduce_subarray", "MPIR_Hip_subarray_plan_info",
    "MPIX_Reduce_local_fetch", "MPIR_Hip_reduce_fetch", "MPIR_Hip_fetch_plan_info",
    "MPIX_Reduce_local_indexed", "MPIR_Hip_reduce_indexed", "MPIR_Hip_indexed_plan_info",
    "MPIX_Reduce_local_indexed_ordered", "MPIR_Hip_reduce_indexed_ordered", "MPIR_Hip_indexed_ordered_plan_info",
    "MPIX_Reduce_local_order", "MPIX_Reduce_local_order_worksize", "MPIR_Hip_order_build", "MPIR_Hip_order_worksize",
    "MPIX_Reduce_local_indexed_chunked", "MPIX_Reduce_local_chunked_worksize", "MPIX_Reduce_local_runs",
    "MPIR_Hip_reduce_indexed_chunked", "MPIR_Hip_indexed_chunked_plan_info", "MPIR_Hip_chunked_worksize",
    "MPIR_Hip_runs_build",
    "MPIX_Reduce_local_ragged", "MPIR_Hip_reduce_ragged", "MPIR_Hip_ragged_plan_info",
    "MPIX_Reduce_local_fetch_ragged", "MPIR_Hip_reduce_fetch_ragged", "MPIR_Hip_fetch_ragged_plan_info",
    "MPIX_Reduce_local_fetch_indexed_ordered", "MPIR_Hip_reduce_fetch_indexed_ordered",
    "MPIR_Hip_fetch_indexed_ordered_plan_info",
    "MPIX_Compare_and_swap_indexed_ordered", "MPIR_Hip_cas_indexed_ordered", "MPIR_Hip_cas_plan_info",
    # device collectives (include/mpix_hip_coll.h)
    "MPIX_Hip_comm_get_unique_id", "MPIX_Hip_comm_create", "MPIX_Hip_comm_create_loopback",
    "MPIX_Hip_comm_free", "MPIX_Hip_comm_rank", "MPIX_Hip_comm_size",
    "MPIX_Allreduce_hip", "MPIX_Reduce_scatter_block_hip", "MPIX_Reduce_hip", "MPIX_Reduce_scatter_hip",
    "MPIX_Scan_hip", "MPIX_Exscan_hip",
    # the HIP shim (include/mpir_hip_reduce.h)
    "MPIR_Hip_reduce", "MPIR_Hip_elem_size", "MPIR_Hip_has_kernel", "MPIR_Hip_is_device_ptr",
    "MPIR_Hip_pointer_kind", "MPIR_Hip_memcpy", "MPIR_Hip_error_string", "MPIR_Hip_device_count", "MPIR_Hip_thread_contexts",
    "MPIR_Hip_host_max_bytes", "MPIR_Hip_set_host_max_bytes", "MPIR_Hip_mixed_max_bytes", "MPIR_Hip_direct_dispatches", "MPIR_Hip_direct_profile",
    "MPIR_Hip_direct_last_kernel_ns", "MPIR_Hip_direct_state", "MPIR_Hip_direct_busy_skips",
    "MPIR_Hip_direct_last_split", "MPIR_Hip_direct_kernarg_writes", "MPIR_Hip_direct_placement", "MPIR_Hip_build_id", "MPIR_Hip_combine_set_flags",
    "MPIR_Hip_direct_prepare", "MPIR_Hip_set_local_ranks", "MPIR_Hip_host_threads",
    "MPIR_Hip_default_rings_in_vram", "MPIR_Hip_direct_ring_location", "MPIR_Hip_set_keep_bytes",
    "MPIR_Hip_set_keep_min_bytes", "MPIR_Hip_plan_info", "MPIR_Hip_combine_plan_info",
    # runtime subset for config 1 (include/mpi_pip.h)
    "MPI_Init", "MPI_Initialized", "MPI_Finalize", "MPI_Finalized", "MPI_Abort", "MPI_Comm_size",
    "MPI_Comm_rank", "MPI_Get_processor_name", "MPI_Wtime", "MPI_Wtick", "MPI_Barrier", "MPI_Bcast",
    "MPI_Reduce",
]

MPI_User_function = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int))



class ReduceLocalSeg(ctypes.Structure):
    """MPIX_Reduce_local_seg (include/mpi_reduce_local.h)."""
    _fields_ = [("inbuf", ctypes.c_void_p), ("inoutbuf", ctypes.c_void_p), ("count", ctypes.c_int)]


class HipSeg(ctypes.Structure):
    """MPIR_Hip_seg (include/mpir_hip_reduce.h)."""
    _fields_ = [("inbuf", ctypes.c_void_p), ("inoutbuf", ctypes.c_void_p), ("count", ctypes.c_uint64)]


_lib = None


# what load()'s MPIR_Hip_default_rings_in_vram(1) returned: 1 set then, 0 the
# environment held a value, -1 the HSA runtime had started (None: not loaded)
RINGS_DEFAULT = None


def load(path: str | None = None) -> ctypes.CDLL:
    """Load the C-ABI library (raises if it was not built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"{p} missing: build it with `make -C mpich-pip_amd` "
                           "(no CPU fallback exists for MPI_Reduce_local)")
    lib = ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name in ("MPI_Reduce_local", "PMPI_Reduce_local", "MPIR_Reduce_local"):
        f = getattr(lib, name)
        f.argtypes = [vp, vp, i32, i32, i32]
        f.restype = i32
    lib.MPIX_Reduce_local_stream.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_stream.restype = i32
    lib.MPIX_Reduce_local_multi.argtypes = [ctypes.POINTER(vp), i32, vp, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_multi.restype = i32
    lib.MPIX_Reduce_local_batch.argtypes = [ctypes.POINTER(ReduceLocalSeg), i32, i32, i32, vp]
    lib.MPIX_Reduce_local_batch.restype = i32
    lib.MPIR_Hip_reduce_batch.argtypes = [ctypes.POINTER(HipSeg), i32, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_batch.restype = i32
    lib.MPIR_Hip_batch_plan_info.argtypes = [ctypes.POINTER(HipSeg), i32, i32, i32, ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    lib.MPIR_Hip_batch_plan_info.restype = i32
    u64 = ctypes.c_uint64
    lib.MPIX_Reduce_local_strided.argtypes = [vp, ctypes.c_long, vp, ctypes.c_long, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_strided.restype = i32
    lib.MPIR_Hip_reduce_strided.argtypes = [vp, u64, vp, u64, u64, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_strided.restype = i32
    lib.MPIR_Hip_strided_plan_info.argtypes = [vp, u64, vp, u64, u64, u64, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_strided_plan_info.restype = i32
    for name in ("MPIR_Hip_set_strided_wide_bytes", "MPIR_Hip_strided_test_max_groups"):
        getattr(lib, name).argtypes = [u64]
        getattr(lib, name).restype = u64
    ip = ctypes.POINTER(i32)
    lib.MPIX_Reduce_local_subarray.argtypes = [vp, ip, ip, vp, ip, ip, i32, ip, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_subarray.restype = i32
    lib.MPIR_Hip_reduce_subarray.argtypes = [vp, ip, ip, vp, ip, ip, i32, ip, i32, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_subarray.restype = i32
    lib.MPIR_Hip_subarray_plan_info.argtypes = [vp, ip, ip, vp, ip, ip, i32, ip, i32, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_subarray_plan_info.restype = i32
    lib.MPIX_Reduce_local_fetch.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_fetch.restype = i32
    lib.MPIR_Hip_reduce_fetch.argtypes = [vp, vp, vp, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_fetch.restype = i32
    lib.MPIR_Hip_fetch_plan_info.argtypes = [vp, vp, vp, u64, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_fetch_plan_info.restype = i32
    lib.MPIX_Reduce_local_indexed.argtypes = [vp, vp, vp, vp, ctypes.c_long, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_indexed.restype = i32
    lib.MPIR_Hip_reduce_indexed.argtypes = [vp, vp, vp, vp, u64, u64, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_indexed.restype = i32
    lib.MPIR_Hip_indexed_plan_info.argtypes = [vp, vp, vp, vp, u64, u64, u64, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_indexed_plan_info.restype = i32
    lib.MPIX_Reduce_local_indexed_ordered.argtypes = [vp, vp, vp, vp, vp, ctypes.c_long, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_indexed_ordered.restype = i32
    lib.MPIR_Hip_reduce_indexed_ordered.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_indexed_ordered.restype = i32
    lib.MPIR_Hip_indexed_ordered_plan_info.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_indexed_ordered_plan_info.restype = i32
    lib.MPIX_Reduce_local_order.argtypes = [vp, i32, vp, vp, ctypes.c_long, vp]
    lib.MPIX_Reduce_local_order.restype = i32
    lib.MPIX_Reduce_local_order_worksize.argtypes = [i32, ctypes.POINTER(ctypes.c_long)]
    lib.MPIX_Reduce_local_order_worksize.restype = i32
    lib.MPIR_Hip_order_build.argtypes = [vp, u64, vp, vp, u64, vp, i32]
    lib.MPIR_Hip_order_build.restype = i32
    lib.MPIR_Hip_order_worksize.argtypes = [u64, ctypes.POINTER(u64)]
    lib.MPIR_Hip_order_worksize.restype = i32
    lib.MPIX_Reduce_local_indexed_chunked.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_long, i32, i32, i32, i32, vp,
                                                      ctypes.c_long, vp]
    lib.MPIX_Reduce_local_indexed_chunked.restype = i32
    lib.MPIX_Reduce_local_chunked_worksize.argtypes = [i32, i32, i32, ctypes.POINTER(ctypes.c_long)]
    lib.MPIX_Reduce_local_chunked_worksize.restype = i32
    lib.MPIX_Reduce_local_runs.argtypes = [vp, vp, i32, vp, vp]
    lib.MPIX_Reduce_local_runs.restype = i32
    lib.MPIR_Hip_reduce_indexed_chunked.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, vp, u64, vp, i32]
    lib.MPIR_Hip_reduce_indexed_chunked.restype = i32
    lib.MPIR_Hip_indexed_chunked_plan_info.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u64, i32, i32,
                                                       ctypes.POINTER(u64)]
    lib.MPIR_Hip_indexed_chunked_plan_info.restype = i32
    lib.MPIR_Hip_chunked_worksize.argtypes = [u64, u64, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_chunked_worksize.restype = i32
    lib.MPIR_Hip_runs_build.argtypes = [vp, vp, u64, vp, vp, i32]
    lib.MPIR_Hip_runs_build.restype = i32
    lib.MPIX_Reduce_local_ragged.argtypes = [vp, vp, vp, vp, vp, ctypes.c_long, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_ragged.restype = i32
    lib.MPIR_Hip_reduce_ragged.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_ragged.restype = i32
    lib.MPIR_Hip_ragged_plan_info.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_ragged_plan_info.restype = i32
    lib.MPIX_Reduce_local_fetch_ragged.argtypes = [vp, vp, vp, vp, vp, ctypes.c_long, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_fetch_ragged.restype = i32
    lib.MPIR_Hip_reduce_fetch_ragged.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_fetch_ragged.restype = i32
    lib.MPIR_Hip_fetch_ragged_plan_info.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_fetch_ragged_plan_info.restype = i32
    lib.MPIX_Reduce_local_fetch_indexed_ordered.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_long, i32, i32, i32, i32, vp]
    lib.MPIX_Reduce_local_fetch_indexed_ordered.restype = i32
    lib.MPIR_Hip_reduce_fetch_indexed_ordered.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce_fetch_indexed_ordered.restype = i32
    lib.MPIR_Hip_fetch_indexed_ordered_plan_info.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u64, i32, i32,
                                                             ctypes.POINTER(u64)]
    lib.MPIR_Hip_fetch_indexed_ordered_plan_info.restype = i32
    lib.MPIX_Compare_and_swap_indexed_ordered.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_long, i32, i32, vp]
    lib.MPIX_Compare_and_swap_indexed_ordered.restype = i32
    lib.MPIR_Hip_cas_indexed_ordered.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, vp, i32]
    lib.MPIR_Hip_cas_indexed_ordered.restype = i32
    lib.MPIR_Hip_cas_plan_info.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, ctypes.POINTER(u64)]
    lib.MPIR_Hip_cas_plan_info.restype = i32
    lib.MPIX_Hip_comm_get_unique_id.argtypes = [vp]
    lib.MPIX_Hip_comm_get_unique_id.restype = i32
    lib.MPIX_Hip_comm_create.argtypes = [vp, i32, i32, ctypes.POINTER(vp)]
    lib.MPIX_Hip_comm_create.restype = i32
    lib.MPIX_Hip_comm_create_loopback.argtypes = [i32, ctypes.POINTER(vp)]
    lib.MPIX_Hip_comm_create_loopback.restype = i32
    lib.MPIX_Hip_comm_free.argtypes = [ctypes.POINTER(vp)]
    lib.MPIX_Hip_comm_free.restype = i32
    for name in ("MPIX_Allreduce_hip", "MPIX_Reduce_scatter_block_hip", "MPIX_Scan_hip", "MPIX_Exscan_hip"):
        f = getattr(lib, name)
        f.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp]
        f.restype = i32
    lib.MPIX_Reduce_hip.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp]
    lib.MPIX_Reduce_hip.restype = i32
    lib.MPIX_Reduce_scatter_hip.argtypes = [vp, vp, ctypes.POINTER(i32), i32, i32, vp, i32, vp]
    lib.MPIX_Reduce_scatter_hip.restype = i32
    lib.MPIX_Reduce_local_set_errhandler.argtypes = [i32]
    lib.MPIX_Reduce_local_set_errhandler.restype = i32
    lib.MPI_Op_create.argtypes = [MPI_User_function, i32, ctypes.POINTER(i32)]
    lib.MPI_Op_create.restype = i32
    lib.MPI_Op_free.argtypes = [ctypes.POINTER(i32)]
    lib.MPI_Op_free.restype = i32
    lib.MPI_Op_commutative.argtypes = [i32, ctypes.POINTER(i32)]
    lib.MPI_Op_commutative.restype = i32
    lib.MPIR_Op_is_commutative.argtypes = [i32]
    lib.MPIR_Op_is_commutative.restype = i32
    lib.MPI_Error_string.argtypes = [i32, ctypes.c_char_p, ctypes.POINTER(i32)]
    lib.MPI_Error_string.restype = i32
    lib.MPIR_Hip_reduce.argtypes = [vp, vp, ctypes.c_uint64, i32, i32, vp, i32]
    lib.MPIR_Hip_reduce.restype = i32
    lib.MPIR_Hip_has_kernel.argtypes = [i32, i32]
    lib.MPIR_Hip_has_kernel.restype = i32
    lib.MPIR_Hip_elem_size.argtypes = [i32]
    lib.MPIR_Hip_elem_size.restype = ctypes.c_size_t
    lib.MPIR_Hip_device_count.restype = i32
    lib.MPIR_Hip_thread_contexts.restype = i32
    lib.MPIR_Hip_host_max_bytes.restype = ctypes.c_uint64
    lib.MPIR_Hip_set_host_max_bytes.argtypes = [ctypes.c_uint64]
    lib.MPIR_Hip_set_host_max_bytes.restype = ctypes.c_uint64
    lib.MPIR_Hip_mixed_max_bytes.restype = ctypes.c_uint64
    lib.MPIR_Hip_direct_dispatches.restype = ctypes.c_uint64
    lib.MPIR_Hip_direct_profile.argtypes = [i32]
    lib.MPIR_Hip_direct_profile.restype = None
    lib.MPIR_Hip_direct_last_kernel_ns.restype = ctypes.c_uint64
    lib.MPIR_Hip_direct_state.argtypes = [i32]
    lib.MPIR_Hip_direct_state.restype = i32
    lib.MPIR_Hip_direct_busy_skips.restype = ctypes.c_uint64
    lib.MPIR_Hip_direct_kernarg_writes.restype = ctypes.c_uint64
    lib.MPIR_Hip_direct_last_split.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    lib.MPIR_Hip_direct_last_split.restype = None
    lib.MPIR_Hip_direct_placement.argtypes = [i32, ctypes.POINTER(i32)]
    lib.MPIR_Hip_direct_placement.restype = None
    lib.MPIR_Hip_direct_prepare.argtypes = [i32]
    lib.MPIR_Hip_direct_prepare.restype = i32
    lib.MPIR_Hip_default_rings_in_vram.argtypes = [i32]
    lib.MPIR_Hip_default_rings_in_vram.restype = i32
    lib.MPIR_Hip_direct_ring_location.argtypes = [i32]
    lib.MPIR_Hip_direct_ring_location.restype = i32
    for name in ("MPIR_Hip_set_keep_bytes", "MPIR_Hip_set_keep_min_bytes"):
        getattr(lib, name).argtypes = [ctypes.c_uint64]
        getattr(lib, name).restype = ctypes.c_uint64
    lib.MPIR_Hip_plan_info.argtypes = [vp, vp, ctypes.c_uint64, i32, i32, ctypes.POINTER(ctypes.c_uint64)]
    lib.MPIR_Hip_plan_info.restype = i32
    lib.MPIR_Hip_combine_plan_info.argtypes = [ctypes.POINTER(vp), i32, vp, ctypes.c_uint64, i32, i32, i32,
                                               ctypes.POINTER(ctypes.c_uint64)]
    lib.MPIR_Hip_combine_plan_info.restype = i32
    lib.MPIR_Hip_set_local_ranks.argtypes = [i32]
    lib.MPIR_Hip_set_local_ranks.restype = i32
    lib.MPIR_Hip_host_threads.argtypes = []
    lib.MPIR_Hip_host_threads.restype = i32
    lib.MPIR_Hip_build_id.restype = ctypes.c_char_p
    lib.MPIR_Hip_combine_set_flags.argtypes = [i32]
    lib.MPIR_Hip_combine_set_flags.restype = i32
    lib.MPIR_Hip_error_string.restype = ctypes.c_char_p
    lib.MPIR_Hip_pointer_kind.argtypes = [vp, ctypes.c_uint64]
    lib.MPIR_Hip_pointer_kind.restype = i32
    for name in [n for n in EXPORTED_SYMBOLS if n.endswith("_check_dtype")]:
        f = getattr(lib, name)
        f.argtypes = [i32]
        f.restype = i32
    # AQL rings in VRAM (direct_dispatch.hip default_rings_in_vram): the load-time
    # constructor stands aside in a process that already runs threads, which an
    # interpreter that imported numpy or torch first does (their pools are
    # parked and leave the environment alone); load() applies the default then,
    # while the HSA runtime has not started and the job set no value.
    global RINGS_DEFAULT
    RINGS_DEFAULT = lib.MPIR_Hip_default_rings_in_vram(1)
    if RINGS_DEFAULT == 1:
        os.environ["HSA_ALLOCATE_QUEUE_DEV_MEM"] = "1"      # Python's view of the variable the library set
    elif RINGS_DEFAULT == -1 and path is None:
        import warnings
        warnings.warn("mpich_pip_amd loaded after the GPU runtime started: its AQL rings stay in host memory "
                      "(~1.7 us per synchronous call); load it before the first GPU call, or export "
                      "HSA_ALLOCATE_QUEUE_DEV_MEM=1 (INTEGRATION.md, 'Keep the AQL rings in VRAM')",
                      RuntimeWarning, stacklevel=2)
    if path is None:
        _lib = lib
    return lib


def build_id() -> str:
    """MPIR_Hip_build_id: the source hashes and commit the library was built from."""
    return load().MPIR_Hip_build_id().decode()


def placement(dev: int = 0) -> dict:
    """MPIR_Hip_direct_placement for the calling thread: its CPU and NUMA node,
    device `dev`'s node, and the nodes of this thread's completion signal and of
    the device's error word (-1 where unknown or not yet created); `ring_in_vram`:
    MPIR_Hip_direct_ring_location (1 device memory, 0 host memory, -1 no queue)."""
    lib = load()
    out = (ctypes.c_int * 5)()
    lib.MPIR_Hip_direct_placement(dev, out)
    return {"cpu": out[0], "cpu_node": out[1], "gpu_node": out[2], "signal_node": out[3], "error_word_node": out[4],
            "ring_in_vram": lib.MPIR_Hip_direct_ring_location(dev)}


def error_class(code: int) -> int:
    """MPI_Error_class: the class of an error code (codes carry an error-stack
    index above the class bits, as MPICH's do)."""
    c = ctypes.c_int(-1)
    load().MPI_Error_class(code, ctypes.byref(c))
    return c.value


def error_string(code: int) -> str:
    lib = load()
    buf = ctypes.create_string_buffer(512)
    n = ctypes.c_int(0)
    lib.MPI_Error_string(code, buf, ctypes.byref(n))
    return buf.value.decode(errors="replace")


def fast_reduce_local():
    """The compiled binding of MPI_Reduce_local (csrc/py/fastcall.c, METH_FASTCALL):
    f(inbuf, inoutbuf, count, datatype, op) -> error code, ~0.25 us of Python
    overhead per call against ~1.2 us through ctypes.  Same library instance as
    load() (it is loaded first, so the errhandler and per-thread state are shared).
    Raises if the extension was not built."""
    load()
    from . import _fastcall
    return _fastcall.reduce_local


def fast_reduce_local_loop():
    """f(arg_sets, start, k) -> error code: k MPI_Reduce_local calls in a C loop
    (csrc/py/fastcall.c), call i with arg_sets[(start + i) % len(arg_sets)], the
    way a C caller issues them.  Raises if the extension was not built."""
    load()
    from . import _fastcall
    return _fastcall.reduce_local_loop


def reduce_local(inbuf: int, inoutbuf: int, count: int, datatype: int, op: int) -> int:
    """MPI_Reduce_local on raw addresses (device or host)."""
    return load().MPI_Reduce_local(ctypes.c_void_p(inbuf), ctypes.c_void_p(inoutbuf), count, datatype, op)


MPIX_ORDER_TREE = 0
MPIX_ORDER_CHAIN = 1


def reduce_local_multi(inbufs, outbuf: int, count: int, datatype: int, op: int, order: int,
                       stream: int = 0) -> int:
    """MPIX_Reduce_local_multi: outbuf = tree/chain fold of device buffers (addresses)."""
    arr = (ctypes.c_void_p * len(inbufs))(*inbufs)
    return load().MPIX_Reduce_local_multi(arr, len(inbufs), ctypes.c_void_p(outbuf), count, datatype, op, order,
                                          ctypes.c_void_p(stream or None))


# ---- plan introspection (include/mpir_hip_reduce.h; for tests and tools)
# element class (enum MPIR_Hip_elem) of each datatype, as csrc/host/op_kernels.c maps them
_ELEMS = ["I8", "U8", "I16", "U16", "I32", "U32", "I64", "U64", "F16", "F32", "F64", "CF32", "CF64", "P2INT",
          "PFLOATINT", "PLONGINT", "PSHORTINT", "PDOUBLEINT", "F80", "CF80", "PLDOUBLEINT"]
ELEM = {name: i + 1 for i, name in enumerate(_ELEMS)}
ELEM_OF = {
    "MPI_INT": "I32", "MPI_LONG": "I64", "MPI_SHORT": "I16", "MPI_UNSIGNED_SHORT": "U16", "MPI_UNSIGNED": "U32",
    "MPI_UNSIGNED_LONG": "U64", "MPI_LONG_LONG": "I64", "MPI_UNSIGNED_LONG_LONG": "U64", "MPI_SIGNED_CHAR": "I8",
    "MPI_UNSIGNED_CHAR": "U8", "MPI_INT8_T": "I8", "MPI_INT16_T": "I16", "MPI_INT32_T": "I32", "MPI_INT64_T": "I64",
    "MPI_UINT8_T": "U8", "MPI_UINT16_T": "U16", "MPI_UINT32_T": "U32", "MPI_UINT64_T": "U64", "MPI_CHAR": "I8",
    "MPI_AINT": "I64", "MPI_OFFSET": "I64", "MPI_COUNT": "I64", "MPI_FLOAT": "F32", "MPI_DOUBLE": "F64",
    "MPI_LONG_DOUBLE": "F80", "MPIX_C_FLOAT16": "F16", "MPI_C_BOOL": "U8", "MPI_C_FLOAT_COMPLEX": "CF32",
    "MPI_C_DOUBLE_COMPLEX": "CF64", "MPI_C_LONG_DOUBLE_COMPLEX": "CF80", "MPI_BYTE": "U8", "MPI_2INT": "P2INT",
    "MPI_FLOAT_INT": "PFLOATINT", "MPI_LONG_INT": "PLONGINT", "MPI_SHORT_INT": "PSHORTINT",
    "MPI_DOUBLE_INT": "PDOUBLEINT", "MPI_LONG_DOUBLE_INT": "PLDOUBLEINT",
}
_ELEM_BY_HANDLE = {DATATYPES[t]: ELEM[e] for t, e in ELEM_OF.items()}
PLAN_LEAN, PLAN_FULL, PLAN_SHIFT, PLAN_ELEMS, PLAN_ELEMS_U, PLAN_WIDE_TILE, PLAN_WIDE_ELEMS = range(7)
PLAN_NAMES = ["lean", "full", "shift", "elems", "elems_u", "wide_tile", "wide_elems"]
COMBINE_COPY, COMBINE_FUSED_VECTOR, COMBINE_FUSED_ELEMENTS, COMBINE_ANY = range(4)


def plan_info(inbuf: int, inoutbuf: int, count: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_plan_info: the launch plan of a device-resident MPI_Reduce_local
    at these addresses (never dereferenced; no GPU needed).  `datatype` and `op`
    are MPI handles.  Raises where the pair has no planned kernel."""
    out = (ctypes.c_uint64 * 6)()
    rc = load().MPIR_Hip_plan_info(ctypes.c_void_p(inbuf), ctypes.c_void_p(inoutbuf), count, op & 0xFF,
                                   _ELEM_BY_HANDLE[datatype], out)
    if rc:
        raise LookupError(f"MPIR_Hip_plan_info: {rc}")
    return dict(zip(("kind", "groups", "nhead", "ntail", "vbytes", "keep"), (int(v) for v in out)))


def combine_plan_info(inbufs, outbuf: int, count: int, datatype: int, op: int, order: int) -> dict:
    """MPIR_Hip_combine_plan_info: the path of a fold of device buffers at these
    addresses (never dereferenced; no GPU needed)."""
    arr = (ctypes.c_void_p * len(inbufs))(*inbufs)
    out = (ctypes.c_uint64 * 4)()
    rc = load().MPIR_Hip_combine_plan_info(arr, len(inbufs), ctypes.c_void_p(outbuf), count, op & 0xFF,
                                           _ELEM_BY_HANDLE[datatype], order, out)
    if rc:
        raise LookupError(f"MPIR_Hip_combine_plan_info: {rc}")
    return dict(zip(("path", "passes", "nhead", "ntail"), (int(v) for v in out)))


# ---- batched reductions (MPIX_Reduce_local_batch)
BATCH_SEG_EMPTY, BATCH_SEG_TILE, BATCH_SEG_ELEMS, BATCH_SEG_SINGLE = range(4)
BATCH_SEG_NAMES = ["empty", "tile", "elems", "single"]
BATCH_MAX_GROUPS = 1 << 23      # MPIR_HIP_BATCH_MAX_GROUPS: a launch closes before its workgroups pass it


def reduce_local_batch(segs, datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_batch: `segs` is an iterable of (inbuf, inoutbuf, count)
    on raw device addresses; one launch combines them all.  stream 0: synchronous
    on the library stream; otherwise enqueued on that HIP stream, no wait."""
    segs = list(segs)
    arr = (ReduceLocalSeg * max(len(segs), 1))(*[ReduceLocalSeg(i or None, o or None, n) for i, o, n in segs])
    return load().MPIX_Reduce_local_batch(arr, len(segs), datatype, op, ctypes.c_void_p(stream or None))


def batch_plan_info(segs, datatype: int, op: int) -> dict:
    """MPIR_Hip_batch_plan_info: the launches of a batch of device segments at
    these addresses (never dereferenced; no GPU needed): launches, groups (over
    all launches), tile / elems / empty (segments per path), max_segs (per
    launch), and per segment seg_kind (BATCH_SEG_*) and seg_groups.  Raises where
    the pair has no batch kernel."""
    segs = list(segs)
    n = len(segs)
    arr = (HipSeg * max(n, 1))(*[HipSeg(i or None, o or None, c) for i, o, c in segs])
    out = (ctypes.c_uint64 * 6)()
    kind, groups = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
    rc = load().MPIR_Hip_batch_plan_info(arr, n, op & 0xFF, _ELEM_BY_HANDLE[datatype], out, kind, groups)
    if rc:
        raise LookupError(f"MPIR_Hip_batch_plan_info: {rc}")
    d = dict(zip(("launches", "groups", "tile", "elems", "empty", "max_segs"), (int(v) for v in out)))
    d["seg_kind"] = [int(kind[i]) for i in range(n)]
    d["seg_groups"] = [int(groups[i]) for i in range(n)]
    return d


# ---- strided reductions (MPIX_Reduce_local_strided)
STRIDED_EMPTY, STRIDED_SINGLE, STRIDED_WIDE, STRIDED_NARROW_VEC, STRIDED_NARROW_ELEMS = range(5)
STRIDED_NAMES = ["empty", "single", "wide", "narrow_vec", "narrow_elems"]
MPIR_HIP_EARG = 5


def reduce_local_strided(inbuf: int, in_stride: int, inoutbuf: int, inout_stride: int, nblocks: int, blocklen: int,
                         datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_strided: nblocks rows of blocklen elements, row r at
    inbuf + r * in_stride and inoutbuf + r * inout_stride (raw device addresses,
    strides in bytes), in one launch.  stream 0: synchronous on the library
    stream; otherwise enqueued on that HIP stream, no wait."""
    return load().MPIX_Reduce_local_strided(ctypes.c_void_p(inbuf or None), in_stride, ctypes.c_void_p(inoutbuf or None),
                                            inout_stride, nblocks, blocklen, datatype, op,
                                            ctypes.c_void_p(stream or None))


def strided_plan_info(inbuf: int, in_stride: int, inoutbuf: int, inout_stride: int, nblocks: int, blocklen: int,
                      datatype: int, op: int) -> dict:
    """MPIR_Hip_strided_plan_info: the launches of a strided reduction of device
    operands at these addresses (never dereferenced; no GPU needed): form
    (STRIDED_*), launches, groups (over all launches), per (WIDE: G, workgroups
    per row; NARROW: units per workgroup), tile_rows / elem_rows (WIDE: rows per
    path), threshold (bytes from which a row is wide) and rows_per_launch.
    Raises LookupError where the pair has no kernel, ValueError for strides the
    call refuses."""
    out = (ctypes.c_uint64 * 8)()
    rc = load().MPIR_Hip_strided_plan_info(ctypes.c_void_p(inbuf or None), in_stride, ctypes.c_void_p(inoutbuf or None),
                                           inout_stride, nblocks, blocklen, op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_strided_plan_info: strides refused")
    if rc:
        raise LookupError(f"MPIR_Hip_strided_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "tile_rows", "elem_rows", "threshold", "rows_per_launch"),
                    (int(v) for v in out)))


# ---- subarray reductions (MPIX_Reduce_local_subarray)
MPI_ERR_DIMS = 11
MPI_ORDER_C, MPI_ORDER_FORTRAN = 56, 57
SUBARRAY_MAXDIMS = 8
SUBARRAY_SINGLE, SUBARRAY_WIDE, SUBARRAY_NARROW_VEC, SUBARRAY_NARROW_ELEMS, SUBARRAY_STRIDED = range(1, 6)
SUBARRAY_NAMES = ["", "single", "wide", "narrow_vec", "narrow_elems", "strided"]


def _ints(seq):
    """An int array for the C ABI, or None (a packed operand's sizes and starts)."""
    return None if seq is None else (ctypes.c_int * max(len(seq), 1))(*seq)


def reduce_local_subarray(inbuf: int, in_sizes, in_starts, inoutbuf: int, inout_sizes, inout_starts, subsizes,
                          order: int, datatype: int, op: int, stream: int = 0, ndims: int | None = None) -> int:
    """MPIX_Reduce_local_subarray: the sub-box subsizes of the array in_sizes at
    in_starts combined into the one of inout_sizes at inout_starts (raw device
    addresses of the arrays' origins; sequences of ints; sizes None: that side is
    packed).  ndims defaults to len(subsizes).  stream 0: synchronous on the
    library stream; otherwise enqueued on that HIP stream, no wait."""
    n = len(subsizes) if ndims is None else ndims
    return load().MPIX_Reduce_local_subarray(ctypes.c_void_p(inbuf or None), _ints(in_sizes), _ints(in_starts),
                                             ctypes.c_void_p(inoutbuf or None), _ints(inout_sizes), _ints(inout_starts),
                                             n, _ints(subsizes), order, datatype, op, ctypes.c_void_p(stream or None))


def subarray_plan_info(inbuf: int, in_sizes, in_starts, inoutbuf: int, inout_sizes, inout_starts, subsizes, order: int,
                       datatype: int, op: int) -> dict:
    """MPIR_Hip_subarray_plan_info: the normal form and the launches of a subarray
    reduction of device operands at these addresses (never dereferenced; no GPU
    needed): form (SUBARRAY_*), launches, groups (over all launches), per (WIDE:
    G; NARROW: units per workgroup), units_per_row (NARROW), threshold,
    rows_per_launch, k, blocklen, in_offset / io_offset (bytes from the arrays'
    origins to the boxes), n / in_stride / io_stride (the k outer dimensions,
    fastest first, strides in bytes) and, for SUBARRAY_STRIDED, strided_form,
    tile_rows and elem_rows as strided_plan_info reports them.  Raises LookupError
    where the pair has no kernel, ValueError for arguments the call refuses."""
    out = (ctypes.c_uint64 * 40)()
    rc = load().MPIR_Hip_subarray_plan_info(ctypes.c_void_p(inbuf or None), _ints(in_sizes), _ints(in_starts),
                                            ctypes.c_void_p(inoutbuf or None), _ints(inout_sizes), _ints(inout_starts),
                                            len(subsizes), _ints(subsizes), int(order == MPI_ORDER_C), op & 0xFF,
                                            _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_subarray_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_subarray_plan_info: {rc}")
    d = dict(zip(("form", "launches", "groups", "per", "units_per_row", "threshold", "rows_per_launch", "k", "blocklen",
                  "in_offset", "io_offset", "strided_form", "tile_rows", "elem_rows"), (int(v) for v in out)))
    k = d["k"]
    d["n"] = [int(out[16 + j]) for j in range(k)]
    d["in_stride"] = [int(out[24 + j]) for j in range(k)]
    d["io_stride"] = [int(out[32 + j]) for j in range(k)]
    return d


# ---- fetching reductions (MPIX_Reduce_local_fetch)
FETCH_EMPTY, FETCH_COPY, FETCH_TILE, FETCH_ELEMS = range(4)
FETCH_NAMES = ["empty", "copy", "tile", "elems"]


def reduce_local_fetch(inbuf: int, inoutbuf: int, fetchbuf: int, count: int, datatype: int, op: int,
                       stream: int = 0) -> int:
    """MPIX_Reduce_local_fetch on raw device addresses: fetchbuf receives the bytes
    inoutbuf held, inoutbuf the combine, in one launch.  MPI_NO_OP and MPI_REPLACE
    are accepted (inbuf may be 0 under MPI_NO_OP).  stream 0: synchronous on the
    library stream; otherwise enqueued on that HIP stream, no wait."""
    return load().MPIX_Reduce_local_fetch(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(inoutbuf or None),
                                          ctypes.c_void_p(fetchbuf or None), count, datatype, op,
                                          ctypes.c_void_p(stream or None))


def fetch_plan_info(inbuf: int, inoutbuf: int, fetchbuf: int, count: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_fetch_plan_info: the plan of a fetching reduction of device operands
    at these addresses (never dereferenced; no GPU needed): path (FETCH_*), groups
    (the one launch's workgroups; 0 for empty and copy) and the nhead / ntail
    elements of the tile path.  Raises LookupError where the pair has no kernel."""
    out = (ctypes.c_uint64 * 4)()
    rc = load().MPIR_Hip_fetch_plan_info(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(inoutbuf or None),
                                         ctypes.c_void_p(fetchbuf or None), count, op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc:
        raise LookupError(f"MPIR_Hip_fetch_plan_info: {rc}")
    return dict(zip(("path", "groups", "nhead", "ntail"), (int(v) for v in out)))


# ---- indexed reductions (MPIX_Reduce_local_indexed)
INDEXED_EMPTY, INDEXED_SINGLE, INDEXED_WIDE, INDEXED_NARROW_VEC, INDEXED_NARROW_ELEMS = range(5)
INDEXED_NAMES = ["empty", "single", "wide", "narrow_vec", "narrow_elems"]


def _table_addr(table) -> int:
    """A displacement table's address: None / 0 (no table), a raw address (device
    memory, or host memory for the synchronous call), or a C-contiguous numpy
    int64 array (a host table; the caller keeps it alive over the call)."""
    if table is None or isinstance(table, int):
        return table or 0
    if str(table.dtype) != "int64" or not table.flags["C_CONTIGUOUS"]:
        raise TypeError("a displacement table is a C-contiguous int64 array (MPI_Aint)")
    return table.ctypes.data


def reduce_local_indexed(inbuf: int, in_displs, inoutbuf: int, inout_displs, disp_unit: int, nblocks: int,
                         blocklen: int, datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_indexed: nblocks blocks of blocklen elements, block k at
    inbuf + in_displs[k] * disp_unit and inoutbuf + inout_displs[k] * disp_unit
    bytes (raw device addresses; a table None: that side packed), in one launch.
    A table is a raw address or a numpy int64 array (see _table_addr).  stream 0:
    synchronous on the library stream (host tables allowed); otherwise enqueued on
    that HIP stream, no wait (device tables only)."""
    return load().MPIX_Reduce_local_indexed(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None),
                                            ctypes.c_void_p(inoutbuf or None),
                                            ctypes.c_void_p(_table_addr(inout_displs) or None), disp_unit, nblocks,
                                            blocklen, datatype, op, ctypes.c_void_p(stream or None))


def indexed_plan_info(inbuf: int, in_displs, inoutbuf: int, inout_displs, disp_unit: int, nblocks: int, blocklen: int,
                      datatype: int, op: int) -> dict:
    """MPIR_Hip_indexed_plan_info: the launches of an indexed reduction of device
    operands and tables at these addresses (never dereferenced, the tables only
    compared with 0; no GPU needed): form (INDEXED_*), launches, groups (over all
    launches), per (WIDE: G, workgroups per block; NARROW: units per workgroup),
    threshold (bytes from which a block is wide) and rows_per_launch.  Raises
    LookupError where the pair has no kernel, ValueError for arguments the call
    refuses."""
    out = (ctypes.c_uint64 * 6)()
    rc = load().MPIR_Hip_indexed_plan_info(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None),
                                           ctypes.c_void_p(inoutbuf or None),
                                           ctypes.c_void_p(_table_addr(inout_displs) or None), disp_unit, nblocks,
                                           blocklen, op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_indexed_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_indexed_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "threshold", "rows_per_launch"), (int(v) for v in out)))


# ---- ordered indexed reductions (MPIX_Reduce_local_indexed_ordered)
def _order_addr(order) -> int:
    """An order table's address: None / 0 (no table), a raw address, or a
    C-contiguous numpy int32 array (a host table; the caller keeps it alive)."""
    if order is None or isinstance(order, int):
        return order or 0
    if str(order.dtype) != "int32" or not order.flags["C_CONTIGUOUS"]:
        raise TypeError("an order table is a C-contiguous int32 array (int)")
    return order.ctypes.data


def reduce_local_indexed_ordered(inbuf: int, in_displs, inoutbuf: int, inout_displs, order, disp_unit: int,
                                 nblocks: int, blocklen: int, datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_indexed_ordered: reduce_local_indexed whose inout_displs
    may repeat, the blocks of one target applied in table order.  order: the
    stable argsort of inout_displs as int32 (a raw address or a numpy array, see
    _order_addr; reduce_local_order makes one); None: the indexed call."""
    return load().MPIX_Reduce_local_indexed_ordered(
        ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None), ctypes.c_void_p(inoutbuf or None),
        ctypes.c_void_p(_table_addr(inout_displs) or None), ctypes.c_void_p(_order_addr(order) or None), disp_unit,
        nblocks, blocklen, datatype, op, ctypes.c_void_p(stream or None))


def reduce_local_order_worksize(nblocks: int) -> int:
    """MPIX_Reduce_local_order_worksize: the bytes of scratch reduce_local_order
    may use for nblocks (no GPU needed).  Raises ValueError where it refuses."""
    out = ctypes.c_long(0)
    rc = load().MPIX_Reduce_local_order_worksize(nblocks, ctypes.byref(out))
    if rc:
        raise ValueError(f"MPIX_Reduce_local_order_worksize: {error_string(rc)}")
    return int(out.value)


def reduce_local_order(displs, nblocks: int, order, work: int = 0, work_bytes: int = 0, stream: int = 0) -> int:
    """MPIX_Reduce_local_order: order = the stable argsort of displs[0:nblocks].
    displs: a raw address or a numpy int64 array; order: a raw address or a numpy
    int32 array (written); work: a raw device address of work_bytes bytes, or 0
    (the library's own buffer: the synchronous call only)."""
    return load().MPIX_Reduce_local_order(ctypes.c_void_p(_table_addr(displs) or None), nblocks,
                                          ctypes.c_void_p(_order_addr(order) or None), ctypes.c_void_p(work or None),
                                          work_bytes, ctypes.c_void_p(stream or None))


def indexed_ordered_plan_info(inbuf: int, in_displs, inoutbuf: int, inout_displs, order, disp_unit: int, nblocks: int,
                              blocklen: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_indexed_ordered_plan_info: indexed_plan_info's outputs for the
    launches of the ordered call (rows are sorted positions; order is only
    compared with 0).  Raises as indexed_plan_info does."""
    out = (ctypes.c_uint64 * 6)()
    rc = load().MPIR_Hip_indexed_ordered_plan_info(
        ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None), ctypes.c_void_p(inoutbuf or None),
        ctypes.c_void_p(_table_addr(inout_displs) or None), ctypes.c_void_p(_order_addr(order) or None), disp_unit,
        nblocks, blocklen, op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_indexed_ordered_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_indexed_ordered_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "threshold", "rows_per_launch"), (int(v) for v in out)))


# ---- chunked indexed reductions (MPIX_Reduce_local_indexed_chunked)
REDUCE_LOCAL_CHUNK = 64


def reduce_local_indexed_chunked(inbuf: int, in_displs, inoutbuf: int, inout_displs, order, runstart, disp_unit: int,
                                 nblocks: int, blocklen: int, datatype: int, op: int, work: int = 0, work_bytes: int = 0,
                                 stream: int = 0) -> int:
    """MPIX_Reduce_local_indexed_chunked: reduce_local_indexed_ordered's operands,
    the blocks of one target folded in chunks of REDUCE_LOCAL_CHUNK counted from
    the run's first block, then the partials into the target.  order and runstart:
    int32 tables (raw addresses or numpy arrays, see _order_addr; reduce_local_order
    and reduce_local_runs make them); both None: the indexed call.  work: a raw
    device address of work_bytes bytes (reduce_local_chunked_worksize), or 0 (the
    library's own buffer: the synchronous call only)."""
    return load().MPIX_Reduce_local_indexed_chunked(
        ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None), ctypes.c_void_p(inoutbuf or None),
        ctypes.c_void_p(_table_addr(inout_displs) or None), ctypes.c_void_p(_order_addr(order) or None),
        ctypes.c_void_p(_order_addr(runstart) or None), disp_unit, nblocks, blocklen, datatype, op,
        ctypes.c_void_p(work or None), work_bytes, ctypes.c_void_p(stream or None))


def reduce_local_chunked_worksize(nblocks: int, blocklen: int, datatype: int) -> int:
    """MPIX_Reduce_local_chunked_worksize: the bytes of scratch
    reduce_local_indexed_chunked may use (no GPU needed).  Raises ValueError where
    it refuses."""
    out = ctypes.c_long(0)
    rc = load().MPIX_Reduce_local_chunked_worksize(nblocks, blocklen, datatype, ctypes.byref(out))
    if rc:
        raise ValueError(f"MPIX_Reduce_local_chunked_worksize: {error_string(rc)}")
    return int(out.value)


def reduce_local_runs(displs, order, nblocks: int, runstart, stream: int = 0) -> int:
    """MPIX_Reduce_local_runs: runstart[p] = the first sorted position of the run
    position p lies in.  displs: a raw address or a numpy int64 array; order and
    runstart (written): raw addresses or numpy int32 arrays."""
    return load().MPIX_Reduce_local_runs(ctypes.c_void_p(_table_addr(displs) or None),
                                         ctypes.c_void_p(_order_addr(order) or None), nblocks,
                                         ctypes.c_void_p(_order_addr(runstart) or None), ctypes.c_void_p(stream or None))


def indexed_chunked_plan_info(inbuf: int, in_displs, inoutbuf: int, inout_displs, order, runstart, disp_unit: int,
                              nblocks: int, blocklen: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_indexed_chunked_plan_info: indexed_ordered_plan_info's outputs for
    ONE of the chunked call's two kernels (they share form, launches and groups),
    then total_launches (both kernels) and work_bytes.  Raises as
    indexed_plan_info does."""
    out = (ctypes.c_uint64 * 8)()
    rc = load().MPIR_Hip_indexed_chunked_plan_info(
        ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None), ctypes.c_void_p(inoutbuf or None),
        ctypes.c_void_p(_table_addr(inout_displs) or None), ctypes.c_void_p(_order_addr(order) or None),
        ctypes.c_void_p(_order_addr(runstart) or None), disp_unit, nblocks, blocklen, op & 0xFF,
        _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_indexed_chunked_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_indexed_chunked_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "threshold", "rows_per_launch", "total_launches", "work_bytes"),
                    (int(v) for v in out)))


# ---- ragged reductions (MPIX_Reduce_local_ragged)
RAGGED_EMPTY, RAGGED_SINGLE, RAGGED_RAGGED = range(3)
RAGGED_NAMES = ["empty", "single", "ragged"]


def reduce_local_ragged(inbuf: int, in_displs, inoutbuf: int, inout_displs, starts, disp_unit: int, npieces: int,
                        count: int, datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_ragged: npieces pieces, piece k of starts[k + 1] -
    starts[k] elements at inbuf + in_displs[k] * disp_unit and inoutbuf +
    inout_displs[k] * disp_unit bytes (raw device addresses; a table None: that
    side packed, piece k at starts[k] elements), in one launch.  starts has
    npieces + 1 entries, from 0 to count.  Each table is a raw address or a numpy
    int64 array (see _table_addr).  stream 0: synchronous on the library stream
    (host tables allowed); otherwise enqueued on that HIP stream, no wait (device
    tables only)."""
    return load().MPIX_Reduce_local_ragged(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None),
                                           ctypes.c_void_p(inoutbuf or None),
                                           ctypes.c_void_p(_table_addr(inout_displs) or None),
                                           ctypes.c_void_p(_table_addr(starts) or None), disp_unit, npieces, count,
                                           datatype, op, ctypes.c_void_p(stream or None))


def ragged_plan_info(inbuf: int, in_displs, inoutbuf: int, inout_displs, starts, disp_unit: int, npieces: int,
                     count: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_ragged_plan_info: the launch of a ragged reduction of device
    operands and tables at these addresses (never dereferenced, the tables only
    compared with 0; no GPU needed): form (RAGGED_*), launches (1), groups, per
    (packed elements per workgroup), rounds (of the wave-wide search for a
    workgroup's first piece) and lds_entries (piece boundaries a workgroup holds in
    LDS, 4 bytes each).  Raises LookupError where the pair has no kernel,
    ValueError for arguments the call refuses."""
    out = (ctypes.c_uint64 * 6)()
    rc = load().MPIR_Hip_ragged_plan_info(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None),
                                          ctypes.c_void_p(inoutbuf or None),
                                          ctypes.c_void_p(_table_addr(inout_displs) or None),
                                          ctypes.c_void_p(_table_addr(starts) or None), disp_unit, npieces, count,
                                          op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_ragged_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_ragged_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "rounds", "lds_entries"), (int(v) for v in out)))


# ---- fetching ragged reductions (MPIX_Reduce_local_fetch_ragged)
def reduce_local_fetch_ragged(inbuf: int, inoutbuf: int, inout_displs, fetchbuf: int, starts, disp_unit: int,
                              npieces: int, count: int, datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_fetch_ragged: the fetching reduction on a ragged target.
    inbuf and fetchbuf are packed (piece k at starts[k] elements), piece k of the
    target is at inoutbuf + inout_displs[k] * disp_unit bytes (raw device
    addresses): fetchbuf receives the bytes the pieces held, the pieces the
    combine, in one launch that reads the target once.  MPI_NO_OP (a pack; inbuf
    may be 0) and MPI_REPLACE (a swap) are accepted.  inout_displs None: the fetch
    call on count elements.  Each table is a raw address or a numpy int64 array
    (see _table_addr).  stream 0: synchronous on the library stream (host tables
    allowed); otherwise enqueued on that HIP stream, no wait (device tables only)."""
    return load().MPIX_Reduce_local_fetch_ragged(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(inoutbuf or None),
                                                 ctypes.c_void_p(_table_addr(inout_displs) or None),
                                                 ctypes.c_void_p(fetchbuf or None),
                                                 ctypes.c_void_p(_table_addr(starts) or None), disp_unit, npieces,
                                                 count, datatype, op, ctypes.c_void_p(stream or None))


def fetch_ragged_plan_info(inbuf: int, inoutbuf: int, inout_displs, fetchbuf: int, starts, disp_unit: int,
                           npieces: int, count: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_fetch_ragged_plan_info: the launch of a fetching ragged reduction of
    device operands and tables at these addresses (never dereferenced, the tables
    only compared with 0; no GPU needed): form (RAGGED_*), launches, groups, per
    (packed elements per workgroup), rounds (of the wave-wide search), lds_entries
    (piece boundaries a workgroup holds in LDS) and packed_sides_aligned (1: inbuf
    and fetchbuf at multiples of 16, so chunks can move as vectors).  Raises
    LookupError where the pair has no kernel, ValueError for arguments the call
    refuses."""
    out = (ctypes.c_uint64 * 7)()
    rc = load().MPIR_Hip_fetch_ragged_plan_info(ctypes.c_void_p(inbuf or None), ctypes.c_void_p(inoutbuf or None),
                                                ctypes.c_void_p(_table_addr(inout_displs) or None),
                                                ctypes.c_void_p(fetchbuf or None),
                                                ctypes.c_void_p(_table_addr(starts) or None), disp_unit, npieces,
                                                count, op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_fetch_ragged_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_fetch_ragged_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "rounds", "lds_entries", "packed_sides_aligned"),
                    (int(v) for v in out)))


# ---- fetching ordered indexed reductions (MPIX_Reduce_local_fetch_indexed_ordered)
def reduce_local_fetch_indexed_ordered(inbuf: int, in_displs, inoutbuf: int, inout_displs, fetchbuf: int, order,
                                       disp_unit: int, nblocks: int, blocklen: int, datatype: int, op: int,
                                       stream: int = 0) -> int:
    """MPIX_Reduce_local_fetch_indexed_ordered: reduce_local_indexed_ordered that
    also hands out, in block k of the packed fetchbuf, the bytes block k's target
    held after contributions 0 .. k - 1 and before contribution k (reduce_local_fetch
    block by block in table order).  MPI_NO_OP (inbuf and in_displs may be 0 / None)
    and MPI_REPLACE are accepted.  order: as for reduce_local_indexed_ordered, or
    None with inout_displs given: equal entries of inout_displs are adjacent (in
    particular: no repeats).  Both tables None: reduce_local_fetch on nblocks *
    blocklen elements.  Tables and stream as for reduce_local_indexed_ordered."""
    return load().MPIX_Reduce_local_fetch_indexed_ordered(
        ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None), ctypes.c_void_p(inoutbuf or None),
        ctypes.c_void_p(_table_addr(inout_displs) or None), ctypes.c_void_p(fetchbuf or None),
        ctypes.c_void_p(_order_addr(order) or None), disp_unit, nblocks, blocklen, datatype, op,
        ctypes.c_void_p(stream or None))


def fetch_indexed_ordered_plan_info(inbuf: int, in_displs, inoutbuf: int, inout_displs, fetchbuf: int, order,
                                    disp_unit: int, nblocks: int, blocklen: int, datatype: int, op: int) -> dict:
    """MPIR_Hip_fetch_indexed_ordered_plan_info: indexed_ordered_plan_info's outputs
    for the launches of the fetching ordered call (fetchbuf joins the vector
    form's alignment test; the tables are only compared with 0).  Raises as
    indexed_plan_info does."""
    out = (ctypes.c_uint64 * 6)()
    rc = load().MPIR_Hip_fetch_indexed_ordered_plan_info(
        ctypes.c_void_p(inbuf or None), ctypes.c_void_p(_table_addr(in_displs) or None), ctypes.c_void_p(inoutbuf or None),
        ctypes.c_void_p(_table_addr(inout_displs) or None), ctypes.c_void_p(fetchbuf or None),
        ctypes.c_void_p(_order_addr(order) or None), disp_unit, nblocks, blocklen, op & 0xFF, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_fetch_indexed_ordered_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_fetch_indexed_ordered_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "per", "threshold", "rows_per_launch"), (int(v) for v in out)))


# ---- ordered compare-and-swap (MPIX_Compare_and_swap_indexed_ordered)
CAS_EMPTY, CAS_CONTIG_TILE, CAS_CONTIG_ELEMS, CAS_INDEXED = range(4)
CAS_NAMES = ["empty", "contig_tile", "contig_elems", "indexed"]


def compare_and_swap_indexed_ordered(origin: int, compare: int, target: int, target_displs, result: int, order,
                                     disp_unit: int, count: int, datatype: int, stream: int = 0) -> int:
    """MPIX_Compare_and_swap_indexed_ordered: count compare-and-swaps of one element
    each, in table order.  origin, compare and result are packed by entry number
    (raw device addresses); entry k's target is target + target_displs[k] *
    disp_unit bytes.  result[k] receives what the target held before entry k; where
    that equals compare[k] the target receives origin[k].  order: as for
    reduce_local_indexed_ordered, or None with target_displs given: equal entries
    are adjacent.  target_displs None: a contiguous target.  Tables and stream as
    for reduce_local_indexed_ordered."""
    return load().MPIX_Compare_and_swap_indexed_ordered(
        ctypes.c_void_p(origin or None), ctypes.c_void_p(compare or None), ctypes.c_void_p(target or None),
        ctypes.c_void_p(_table_addr(target_displs) or None), ctypes.c_void_p(result or None),
        ctypes.c_void_p(_order_addr(order) or None), disp_unit, count, datatype, ctypes.c_void_p(stream or None))


def cas_plan_info(origin: int, compare: int, target: int, target_displs, result: int, order, disp_unit: int,
                  count: int, datatype: int) -> dict:
    """MPIR_Hip_cas_plan_info: the launches of an ordered compare-and-swap of device
    operands at these addresses (never dereferenced, the tables only compared with
    0; no GPU needed): form (CAS_*), launches, groups, rows_per_launch (sorted
    positions of a full launch), per (entries one workgroup owns), ahead (kCasAhead,
    the positions a run is walked at a time), nhead and ntail (the elements
    workgroup 0 of the tile form takes).  Raises LookupError where the element's
    size has no kernel, ValueError for arguments the call refuses."""
    out = (ctypes.c_uint64 * 8)()
    rc = load().MPIR_Hip_cas_plan_info(
        ctypes.c_void_p(origin or None), ctypes.c_void_p(compare or None), ctypes.c_void_p(target or None),
        ctypes.c_void_p(_table_addr(target_displs) or None), ctypes.c_void_p(result or None),
        ctypes.c_void_p(_order_addr(order) or None), disp_unit, count, _ELEM_BY_HANDLE[datatype], out)
    if rc == MPIR_HIP_EARG:
        raise ValueError("MPIR_Hip_cas_plan_info: arguments refused")
    if rc:
        raise LookupError(f"MPIR_Hip_cas_plan_info: {rc}")
    return dict(zip(("form", "launches", "groups", "rows_per_launch", "per", "ahead", "nhead", "ntail"),
                    (int(v) for v in out)))


MPIX_HIP_ALG_AUTO = 0
MPIX_HIP_ALG_REFERENCE_ORDER = 1
MPIX_HIP_ALG_RCCL = 2
MPI_IN_PLACE = ctypes.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF).value


def comm_create_loopback(size: int):
    """`size` in-process virtual ranks on the current device (one thread each)."""
    arr = (ctypes.c_void_p * size)()
    rc = load().MPIX_Hip_comm_create_loopback(size, arr)
    if rc:
        raise RuntimeError(error_string(rc))
    return [arr[i] for i in range(size)]


def comm_free(comm) -> int:
    c = ctypes.c_void_p(comm)
    return load().MPIX_Hip_comm_free(ctypes.byref(c))


def allreduce(sendbuf, recvbuf: int, count: int, datatype: int, op: int, comm, algorithm: int = 0,
              stream: int = 0) -> int:
    return load().MPIX_Allreduce_hip(ctypes.c_void_p(sendbuf), ctypes.c_void_p(recvbuf), count, datatype, op,
                                     ctypes.c_void_p(comm), algorithm, ctypes.c_void_p(stream or None))


def reduce(sendbuf, recvbuf, count: int, datatype: int, op: int, root: int, comm, algorithm: int = 0,
           stream: int = 0) -> int:
    """MPIX_Reduce_hip (recvbuf significant at the root only; may be 0 elsewhere)."""
    return load().MPIX_Reduce_hip(ctypes.c_void_p(sendbuf), ctypes.c_void_p(recvbuf), count, datatype, op, root,
                                  ctypes.c_void_p(comm), algorithm, ctypes.c_void_p(stream or None))


def scan(sendbuf, recvbuf: int, count: int, datatype: int, op: int, comm, algorithm: int = 0,
         stream: int = 0) -> int:
    return load().MPIX_Scan_hip(ctypes.c_void_p(sendbuf), ctypes.c_void_p(recvbuf), count, datatype, op,
                                ctypes.c_void_p(comm), algorithm, ctypes.c_void_p(stream or None))


def exscan(sendbuf, recvbuf: int, count: int, datatype: int, op: int, comm, algorithm: int = 0,
           stream: int = 0) -> int:
    return load().MPIX_Exscan_hip(ctypes.c_void_p(sendbuf), ctypes.c_void_p(recvbuf), count, datatype, op,
                                  ctypes.c_void_p(comm), algorithm, ctypes.c_void_p(stream or None))


def reduce_scatter(sendbuf, recvbuf: int, recvcounts, datatype: int, op: int, comm, algorithm: int = 0,
                   stream: int = 0) -> int:
    """MPIX_Reduce_scatter_hip (per-rank recvcounts)."""
    arr = (ctypes.c_int * len(recvcounts))(*recvcounts)
    return load().MPIX_Reduce_scatter_hip(ctypes.c_void_p(sendbuf), ctypes.c_void_p(recvbuf), arr, datatype, op,
                                          ctypes.c_void_p(comm), algorithm, ctypes.c_void_p(stream or None))


def reduce_scatter_block(sendbuf, recvbuf: int, recvcount: int, datatype: int, op: int, comm,
                         algorithm: int = 0, stream: int = 0) -> int:
    return load().MPIX_Reduce_scatter_block_hip(ctypes.c_void_p(sendbuf), ctypes.c_void_p(recvbuf), recvcount,
                                                datatype, op, ctypes.c_void_p(comm), algorithm,
                                                ctypes.c_void_p(stream or None))


def reduce_local_stream(inbuf: int, inoutbuf: int, count: int, datatype: int, op: int, stream: int = 0) -> int:
    """MPIX_Reduce_local_stream: enqueue on a HIP stream (0 = library stream), no wait."""
    return load().MPIX_Reduce_local_stream(ctypes.c_void_p(inbuf), ctypes.c_void_p(inoutbuf), count,
                                           datatype, op, ctypes.c_void_p(stream or None))
