"""TEST INFRASTRUCTURE (a helper, not a test module): what the GPU tests of the host paths need to know about the
machine's HIP runtime, and pinned memory for them.

Some machines (virtual ones, for instance) cannot page-lock memory that a process already has: hipHostRegister
fails there, and so does nexrHostRegister on memory outside the library's cache.
hipHostMalloc and nexrHostMemAlloc work everywhere. A test whose subject is the registration of the caller's own
pages (a registration that ends inside a buffer, one that is dropped while the pages stay, neighbours in one page)
asks for `require_caller_registration()` before it does anything else; every other test takes its pinned memory
from here."""
import ctypes
import importlib
import mmap
from functools import lru_cache

import numpy as np
import pytest

NO_REGISTRATION = "hipHostRegister is not supported here"


def _nexr():
    return importlib.import_module("nex-nccl_amd")


HIP_HOST_REGISTER_MAPPED = 2  # hipHostRegisterMapped


@lru_cache(maxsize=1)
def hip_runtime():
    """libamdhip64 through ctypes, with the few entries the tests call themselves."""
    L = ctypes.CDLL("libamdhip64.so")
    L.hipHostRegister.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint]
    L.hipHostUnregister.argtypes = [ctypes.c_void_p]
    L.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    L.hipHostFree.argtypes = [ctypes.c_void_p]
    L.hipPointerGetAttribute.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for name in ("hipHostRegister", "hipHostUnregister", "hipHostMalloc", "hipHostFree", "hipPointerGetAttribute",
                 "hipGetLastError", "hipPeekAtLastError"):
        getattr(L, name).restype = ctypes.c_int
    return L


@lru_cache(maxsize=1)
def registers_caller_memory() -> bool:
    """Whether the runtime itself takes one page of an anonymous mapping: hipHostRegister and hipHostUnregister
    called directly, not through the library under test (asked once per process; the GPU must be initialised).
    A refusal stays as the thread's last error, which hipGetLastError takes away."""
    hip = hip_runtime()
    page = mmap.mmap(-1, mmap.PAGESIZE)
    addr = np.frombuffer(page, dtype=np.uint8).ctypes.data
    if hip.hipHostRegister(addr, mmap.PAGESIZE, HIP_HOST_REGISTER_MAPPED) != 0:
        hip.hipGetLastError()
        return False
    assert hip.hipHostUnregister(addr) == 0
    return True


def require_caller_registration() -> None:
    if not registers_caller_memory():
        pytest.skip(NO_REGISTRATION)


@lru_cache(maxsize=None)
def allocation(nbytes: int) -> np.ndarray:
    """`nbytes` from nexrHostMemAlloc as a uint8 array, kept for the process (one per size)."""
    addr = _nexr().host_mem_alloc(nbytes)
    return np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * nbytes).from_address(addr))


def registered_memory(nbytes: int):
    """Where ring_host_cases' `registered` kind lives: None (the test's own mapping, registered whole) where the
    runtime page-locks the caller's pages, else an allocation of `nbytes` from nexrHostMemAlloc, inside which
    nexrHostRegister shares the allocation's cache entry."""
    return None if registers_caller_memory() else allocation(nbytes)
