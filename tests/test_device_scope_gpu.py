"""The device a call runs on is the operands', not the caller's current one,
and the caller's current device is the same after the call as before it
(shim_ctx.hpp DeviceScope): with device 0 current and every buffer on device 1,
MPIR_Hip_reduce (the element path and the tile path with head and tail),
MPIR_Hip_combine and MPIR_Hip_reduce_batch each give the host's fp32 sums
bit-exact and leave device 0 current -- in torch's view and in that of the HIP
runtime the library links.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two(mpi, cuda):
    lib = mpi.load()
    if lib.MPIR_Hip_device_count() < 2 or cuda.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    hip = ctypes.CDLL("libamdhip64.so.7")       # the runtime the library links (already loaded by it)
    cuda.cuda.set_device(0)
    assert hip.hipSetDevice(0) == 0
    lib.MPIR_Hip_combine.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.MPIR_Hip_combine.restype = ctypes.c_int
    return lib, hip


def operands(torch, n, seed, k=2):
    """k host fp32 arrays of n elements and their copies on device 1"""
    rng = np.random.default_rng(seed)
    host = [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(k)]
    dev = [torch.from_numpy(h).to("cuda:1") for h in host]
    torch.cuda.synchronize(1)
    return host, dev


def still_on_device_0(torch, hip):
    cur = ctypes.c_int(-1)
    assert hip.hipGetDevice(ctypes.byref(cur)) == 0
    assert cur.value == 0
    assert torch.cuda.current_device() == 0


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("n", [5, 4099], ids=["elements", "tiles_head_tail"])
def test_reduce_on_other_device(mpi, cuda, two, n):
    lib, hip = two
    (b, a), (db, da) = operands(cuda, n, 10 + n)
    rc = lib.MPIR_Hip_reduce(db.data_ptr(), da.data_ptr(), n, mpi.MPI_SUM & 0xFF, mpi.ELEM["F32"], None, 1)
    assert rc == 0, lib.MPIR_Hip_error_string()
    still_on_device_0(cuda, hip)
    assert np.array_equal(bits(da.cpu().numpy()), bits(b + a))


def test_combine_on_other_device(mpi, cuda, two):
    lib, hip = two
    n = 5
    (y0, y1), (d0, d1) = operands(cuda, n, 20)
    out = cuda.zeros(n, dtype=cuda.float32, device="cuda:1")
    cuda.cuda.synchronize(1)
    ins = (ctypes.c_void_p * 2)(d0.data_ptr(), d1.data_ptr())
    rc = lib.MPIR_Hip_combine(ins, 2, out.data_ptr(), n, mpi.MPI_SUM & 0xFF, mpi.ELEM["F32"], mpi.MPIX_ORDER_TREE,
                              None, 1)
    assert rc == 0, lib.MPIR_Hip_error_string()
    still_on_device_0(cuda, hip)
    assert np.array_equal(bits(out.cpu().numpy()), bits(y0 + y1))


def test_batch_on_other_device(mpi, cuda, two):
    lib, hip = two
    n = 5
    (b0, a0, b1, a1), (db0, da0, db1, da1) = operands(cuda, n, 30, k=4)
    segs = (mpi.HipSeg * 2)(mpi.HipSeg(db0.data_ptr(), da0.data_ptr(), n), mpi.HipSeg(db1.data_ptr(), da1.data_ptr(), n))
    rc = lib.MPIR_Hip_reduce_batch(segs, 2, mpi.MPI_SUM & 0xFF, mpi.ELEM["F32"], None, 1)
    assert rc == 0, lib.MPIR_Hip_error_string()
    still_on_device_0(cuda, hip)
    assert np.array_equal(bits(da0.cpu().numpy()), bits(b0 + a0))
    assert np.array_equal(bits(da1.cpu().numpy()), bits(b1 + a1))
