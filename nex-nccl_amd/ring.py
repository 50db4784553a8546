"""Python view of the CPU-emulated collectives (include/nexr_ring.h, libnexr_ring.so; with
``extras=True`` the opt-in include/nexr_extras.h, libnexr_extras.so).

The ring and tree schedules (runRing of all_reduce.h, reduce_scatter.h, all_gather.h, reduce.h,
broadcast.h; runTreeSplit, all_reduce.h:150-230) and the genericOp slicing / FIFO credit
protocol (src/device/prims_simple.h:111-330) run on host threads in C++; every reduceCopy site calls
the MI355X reduce-copy ABI (or any function with its signature, e.g. a test checker).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

from . import LLFlagRule, NexrError, Result, _check, lib

_HERE = os.path.dirname(os.path.abspath(__file__))
RING_LIB_PATH = os.path.join(_HERE, "libnexr_ring.so")
# Opt-in (make -C nex-nccl_amd/csrc EXTRAS=1): include/nexr_extras.h, a superset of libnexr_ring.so.
EXTRAS_LIB_PATH = os.path.join(_HERE, "libnexr_extras.so")
RING_ABI_SYMBOLS = ("nexrRingCommCreate", "nexrRingAllReduce", "nexrRingReduceScatter", "nexrRingAllGather",
                    "nexrRingReduce", "nexrRingBroadcast", "nexrTreeAllReduce", "nexrRingAllReduceSymmetric",
                    "nexrRingReduceScatterSymmetric", "nexrRingAllGatherSymmetric",
                    "nexrRingAllReduceSymmetricLL", "nexrRingReduceScatterSymmetricLL",
                    "nexrRingAllGatherSymmetricLL",
                    "nexrRingAllReduceFlat", "nexrRingReduceScatterFlat", "nexrRingReduceFlat", "nexrRingCommSetFlat",
                    "nexrTreeAllReduceFlat", "nexrRingBroadcastFlat", "nexrRingAllGatherFlat",
                    "nexrRingGroupStart", "nexrRingGroupEnd", "nexrRingGroupGetStats",
                    "nexrTreeTopology", "nexrRingRedOpCreatePreMulSum", "nexrRingRedOpDestroy",
                    "nexrRingCommGetStepWait", "nexrRingCommGetQueued", "nexrRingCommSetLLGroup",
                    "nexrRingCommSetSimpleGroup", "nexrRingCommSetDirect", "nexrRingCommGetDirect",
                    "nexrRingCommSetLLFlagRule",
                    "nexrRingCommGetLLCleanup", "nexrRingCommDestroy", "nexrPeerRingCommCreate",
                    "nexrPeerRingAllReduce", "nexrPeerRingReduceScatter", "nexrPeerRingAllGather",
                    "nexrPeerRingReduce", "nexrPeerRingBroadcast")
EXTRAS_ABI_SYMBOLS = ("nexrSendRecv", "nexrPeerSendRecv", "nexrRingAllReduceResident",
                      "nexrRingReduceScatterResident", "nexrRingAllGatherResident", "nexrRingReduceResident",
                      "nexrRingBroadcastResident", "nexrTreeAllReduceResident", "nexrPeerRingAllReduceResident")

HOST_MEMORY = 0
DEVICE_MEMORY = 1
PROTO_SIMPLE = 0
PROTO_LL = 1
PROTO_LL128 = 2
FLAT_RING, FLAT_TREE, FLAT_COPIES = 1, 2, 4  # NEXR_FLAT_*: nexrRingCommSetFlat's bits
SCALAR_DEVICE, SCALAR_HOST_IMMEDIATE = 0, 1  # nexrScalarResidence_t (= ncclScalarResidence_t)
NUM_OPS = 5  # nexrNumOps: the first user-created op's handle

REDUCE_COPY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                  ctypes.c_void_p)


class RingConfig(ctypes.Structure):
    _fields_ = [("nRanks", ctypes.c_int), ("buffBytes", ctypes.c_size_t), ("memMode", ctypes.c_int),
                ("fn", ctypes.c_void_p), ("timeoutMs", ctypes.c_int), ("protocol", ctypes.c_int),
                ("llFn", ctypes.c_void_p), ("ll128Fn", ctypes.c_void_p), ("treeRanksPerNode", ctypes.c_int),
                ("treeIndex", ctypes.c_int), ("nChannels", ctypes.c_int)]


class PeerRingConfig(ctypes.Structure):
    _fields_ = [("nRanks", ctypes.c_int), ("rank", ctypes.c_int), ("device", ctypes.c_int),
                ("buffBytes", ctypes.c_size_t), ("protocol", ctypes.c_int), ("timeoutMs", ctypes.c_int),
                ("shmName", ctypes.c_char_p)]


class RingGroupStats(ctypes.Structure):
    """nexrRingGroupStats (include/nexr_ring.h)."""
    _fields_ = [("calls", ctypes.c_uint64), ("groupLaunches", ctypes.c_uint64), ("fillLaunches", ctypes.c_uint64),
                ("singles", ctypes.c_uint64), ("cuts", ctypes.c_uint64)]


class _Group:
    """RingComm.group(): nexrRingGroupStart on entry, nexrRingGroupEnd on exit (also behind an exception, whose
    recorded calls then still run: the depth must come down)."""

    def __init__(self, comm):
        self._comm = comm

    def __enter__(self):
        self._comm.group_start()
        return self._comm

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self._comm.group_end()
        else:
            try:
                self._comm.group_end()
            except NexrError:
                pass
        return False


_libs = {}


def _bind_ring(L: ctypes.CDLL) -> None:
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    arr = ctypes.POINTER(ctypes.c_void_p)
    L.nexrRingCommCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(RingConfig)]
    for name, extra in (("nexrRingAllReduce", [i32]), ("nexrRingReduceScatter", [i32]), ("nexrRingAllGather", []),
                        ("nexrRingReduce", [i32, i32]), ("nexrRingBroadcast", [i32]), ("nexrTreeAllReduce", [i32])):
        getattr(L, name).argtypes = [vp, arr, arr, sz, i32] + extra
    for name, extra in (("nexrPeerRingAllReduce", [i32]), ("nexrPeerRingReduceScatter", [i32]),
                        ("nexrPeerRingAllGather", []), ("nexrPeerRingReduce", [i32, i32]),
                        ("nexrPeerRingBroadcast", [i32])):
        getattr(L, name).argtypes = [vp, vp, vp, sz, i32] + extra
    L.nexrRingAllReduceSymmetric.argtypes = [vp, arr, arr, sz, i32, i32, i32]
    L.nexrRingReduceScatterSymmetric.argtypes = [vp, arr, arr, sz, i32, i32]
    L.nexrRingAllGatherSymmetric.argtypes = [vp, arr, arr, sz, i32]
    L.nexrRingAllReduceSymmetricLL.argtypes = [vp, arr, arr, sz, i32, i32, i32]
    L.nexrRingReduceScatterSymmetricLL.argtypes = [vp, arr, arr, sz, i32, i32, i32]
    L.nexrRingAllGatherSymmetricLL.argtypes = [vp, arr, arr, sz, i32, i32]
    L.nexrRingAllReduceFlat.argtypes = [vp, arr, arr, sz, i32, i32]
    L.nexrRingReduceScatterFlat.argtypes = [vp, arr, arr, sz, i32, i32]
    L.nexrRingReduceFlat.argtypes = [vp, arr, arr, sz, i32, i32, i32]
    L.nexrRingCommSetFlat.argtypes = [vp, i32]
    L.nexrTreeAllReduceFlat.argtypes = [vp, arr, arr, sz, i32, i32]
    L.nexrRingBroadcastFlat.argtypes = [vp, arr, arr, sz, i32, i32]
    L.nexrRingAllGatherFlat.argtypes = [vp, arr, arr, sz, i32]
    L.nexrRingGroupStart.argtypes = [vp]
    L.nexrRingGroupEnd.argtypes = [vp]
    L.nexrRingGroupGetStats.argtypes = [vp, ctypes.POINTER(RingGroupStats), i32]
    L.nexrTreeTopology.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.nexrRingRedOpCreatePreMulSum.argtypes = [vp, ctypes.POINTER(i32), arr, i32, i32]
    L.nexrRingRedOpDestroy.argtypes = [vp, i32]
    L.nexrRingCommGetStepWait.argtypes = [vp, ctypes.POINTER(i32)]
    L.nexrRingCommGetQueued.argtypes = [vp, ctypes.POINTER(i32)]
    L.nexrRingCommSetLLGroup.argtypes = [vp, i32]
    L.nexrRingCommSetSimpleGroup.argtypes = [vp, i32]
    L.nexrRingCommSetDirect.argtypes = [vp, i32]
    L.nexrRingCommGetDirect.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.nexrRingCommSetLLFlagRule.argtypes = [vp, ctypes.POINTER(LLFlagRule)]
    L.nexrRingCommGetLLCleanup.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.nexrPeerRingCommCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(PeerRingConfig)]
    L.nexrRingCommDestroy.argtypes = [vp]
    for name in RING_ABI_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int


def _bind_extras(L: ctypes.CDLL) -> None:
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    arr = ctypes.POINTER(ctypes.c_void_p)
    for name, extra in (("nexrRingAllReduceResident", [i32]), ("nexrTreeAllReduceResident", [i32]),
                        ("nexrRingReduceScatterResident", [i32]), ("nexrRingAllGatherResident", []),
                        ("nexrRingReduceResident", [i32, i32]), ("nexrRingBroadcastResident", [i32])):
        getattr(L, name).argtypes = [vp, arr, arr, sz, i32] + extra
    L.nexrPeerRingAllReduceResident.argtypes = [vp, vp, vp, sz, i32, i32]
    L.nexrSendRecv.argtypes = [vp, arr, ctypes.POINTER(i32), arr, ctypes.POINTER(i32), sz]
    L.nexrPeerSendRecv.argtypes = [vp, vp, i32, vp, i32, sz]
    for name in EXTRAS_ABI_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int


def ring_lib() -> ctypes.CDLL:
    """libnexr_ring.so: the graded callers (include/nexr_ring.h)."""
    if "ring" not in _libs:
        lib()  # libnexr.so first (the ring library links against it)
        if not os.path.exists(RING_LIB_PATH):
            raise NexrError(Result.InternalError, f"{RING_LIB_PATH} not built")
        L = ctypes.CDLL(RING_LIB_PATH)
        _bind_ring(L)
        _libs["ring"] = L
    return _libs["ring"]


def extras_available() -> bool:
    return os.path.exists(EXTRAS_LIB_PATH)


def extras_lib() -> ctypes.CDLL:
    """libnexr_extras.so (opt-in): nexr_ring.h's entry points plus include/nexr_extras.h's."""
    if "extras" not in _libs:
        lib()
        if not extras_available():
            raise NexrError(Result.InvalidUsage, f"{EXTRAS_LIB_PATH} not built (make -C nex-nccl_amd/csrc EXTRAS=1)")
        L = ctypes.CDLL(EXTRAS_LIB_PATH)
        _bind_ring(L)
        _bind_extras(L)
        _libs["extras"] = L
    return _libs["extras"]


class RingComm:
    """N emulated ranks (host threads) of one communicator: ring collectives (ncclAllReduce,
    ncclReduceScatter, ncclAllGather, ncclReduce, ncclBroadcast) and the tree ncclAllReduce, each
    run on all ranks at once (one buffer per rank)."""

    def __init__(self, n_ranks: int, mem_mode: int = HOST_MEMORY, buff_bytes: int = 0,
                 fn_address: Optional[int] = None, timeout_ms: int = 0, protocol: int = PROTO_SIMPLE,
                 ll_fn_address: Optional[int] = None, ll128_fn_address: Optional[int] = None,
                 tree_ranks_per_node: int = 0, tree_index: int = 0, n_channels: int = 0, extras: bool = False):
        """extras=True: the communicator lives in the opt-in libnexr_extras.so, which adds send/recv and
        the device-resident collectives; every call on it goes to that library."""
        cfg = RingConfig(n_ranks, buff_bytes, mem_mode, fn_address or None, timeout_ms, protocol,
                         ll_fn_address or None, ll128_fn_address or None, tree_ranks_per_node, tree_index, n_channels)
        self._L = extras_lib() if extras else ring_lib()
        self.extras = extras
        h = ctypes.c_void_p()
        _check(self._L.nexrRingCommCreate(ctypes.byref(h), ctypes.byref(cfg)), "nexrRingCommCreate")
        self._h = h
        self.n_ranks = n_ranks

    def all_reduce(self, sendbuffs: Sequence[int], recvbuffs: Sequence[int], count: int, datatype: int,
                   op: int) -> None:
        if len(sendbuffs) != self.n_ranks or len(recvbuffs) != self.n_ranks:
            raise NexrError(Result.InvalidArgument, "one send and one recv buffer per rank")
        s = (ctypes.c_void_p * self.n_ranks)(*[int(p) for p in sendbuffs])
        r = (ctypes.c_void_p * self.n_ranks)(*[int(p) for p in recvbuffs])
        _check(self._L.nexrRingAllReduce(self._h, s, r, int(count), int(datatype), int(op)), "nexrRingAllReduce")

    def all_reduce_resident(self, sendbuffs: Sequence[int], recvbuffs: Sequence[int], count: int, datatype: int,
                            op: int) -> None:
        """The same all-reduce as one device-resident launch per GPU (nexrRingAllReduceResident)."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._extras().nexrRingAllReduceResident(self._h, s, r, int(count), int(datatype), int(op)),
               "nexrRingAllReduceResident")

    def tree_all_reduce_resident(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._extras().nexrTreeAllReduceResident(self._h, s, r, int(count), int(datatype), int(op)),
               "nexrTreeAllReduceResident")

    def reduce_scatter_resident(self, sendbuffs, recvbuffs, recvcount: int, datatype: int, op: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._extras().nexrRingReduceScatterResident(self._h, s, r, int(recvcount), int(datatype), int(op)),
               "nexrRingReduceScatterResident")

    def all_gather_resident(self, sendbuffs, recvbuffs, sendcount: int, datatype: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._extras().nexrRingAllGatherResident(self._h, s, r, int(sendcount), int(datatype)),
               "nexrRingAllGatherResident")

    def reduce_resident(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int, root: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._extras().nexrRingReduceResident(self._h, s, r, int(count), int(datatype), int(op), int(root)),
               "nexrRingReduceResident")

    def broadcast_resident(self, sendbuffs, recvbuffs, count: int, datatype: int, root: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._extras().nexrRingBroadcastResident(self._h, s, r, int(count), int(datatype), int(root)),
               "nexrRingBroadcastResident")

    def _arrays(self, sendbuffs, recvbuffs):
        if len(sendbuffs) != self.n_ranks or len(recvbuffs) != self.n_ranks:
            raise NexrError(Result.InvalidArgument, "one send and one recv buffer per rank")
        s = (ctypes.c_void_p * self.n_ranks)(*[int(p) if p else None for p in sendbuffs])
        r = (ctypes.c_void_p * self.n_ranks)(*[int(p) if p else None for p in recvbuffs])
        return s, r

    def reduce_scatter(self, sendbuffs, recvbuffs, recvcount: int, datatype: int, op: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingReduceScatter(self._h, s, r, int(recvcount), int(datatype), int(op)),
               "nexrRingReduceScatter")

    def all_gather(self, sendbuffs, recvbuffs, sendcount: int, datatype: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllGather(self._h, s, r, int(sendcount), int(datatype)), "nexrRingAllGather")

    def reduce(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int, root: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingReduce(self._h, s, r, int(count), int(datatype), int(op), int(root)),
               "nexrRingReduce")

    def broadcast(self, sendbuffs, recvbuffs, count: int, datatype: int, root: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingBroadcast(self._h, s, r, int(count), int(datatype), int(root)), "nexrRingBroadcast")

    def tree_all_reduce(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int) -> None:
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrTreeAllReduce(self._h, s, r, int(count), int(datatype), int(op)), "nexrTreeAllReduce")

    def all_reduce_symmetric(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int,
                             n_blocks: int = 0) -> None:
        """ncclAllReduce as the reference's symmetric kernel RSxLD_AGxST in ONE launch
        (nexrRingAllReduceSymmetric): every element folded by its owner, its own input first, in fp32, and
        stored to every rank's recvbuff; n_blocks (0 = 1) only decides where the passes end. Thread ranks,
        device memory, every rank on one GPU (else InvalidUsage); Sum of float32 / float16 / bfloat16 (else
        InvalidArgument). Touches no connection: mixes with ring and tree calls, queued() stays as it was."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllReduceSymmetric(self._h, s, r, int(count), int(datatype), int(op), int(n_blocks)),
               "nexrRingAllReduceSymmetric")

    def reduce_scatter_symmetric(self, sendbuffs, recvbuffs, recvcount: int, datatype: int, op: int) -> None:
        """ncclReduceScatter as the reference's symmetric kernel ReduceScatter_LD in ONE launch
        (nexrRingReduceScatterSymmetric): recvbuffs[r] receives chunk r of the n_ranks * recvcount elements,
        folded from rank r's own input on, in fp32 with one rounding. In place on chunk r of sendbuffs[r]
        allowed. Usage and argument rules as all_reduce_symmetric; queued() stays as it was."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingReduceScatterSymmetric(self._h, s, r, int(recvcount), int(datatype), int(op)),
               "nexrRingReduceScatterSymmetric")

    def all_gather_symmetric(self, sendbuffs, recvbuffs, sendcount: int, datatype: int) -> None:
        """ncclAllGather as the reference's symmetric kernel AllGather_ST in ONE launch
        (nexrRingAllGatherSymmetric): every recvbuffs[s] receives every rank's sendcount elements in rank
        order, a bit copy; a rank whose sendbuff is its own place in its recvbuff skips that store. Usage rules
        as all_reduce_symmetric; queued() stays as it was."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllGatherSymmetric(self._h, s, r, int(sendcount), int(datatype)),
               "nexrRingAllGatherSymmetric")

    def all_reduce_symmetric_ll(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int,
                                n_blocks: int = 0) -> None:
        """ncclAllReduce as the reference's symmetric LL kernel AllReduce_AGxLL_R in ONE launch
        (nexrRingAllReduceSymmetricLL): every element is rank 0's input plus rank 1's, ... in rank order, in
        fp32 with one rounding, on every rank. The communicator owns the windows (made on first use, sized for
        16 blocks: n_blocks is 0..16). Usage and argument rules as all_reduce_symmetric; a message of 2 GiB or
        more is InvalidArgument; queued() stays as it was."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllReduceSymmetricLL(self._h, s, r, int(count), int(datatype), int(op), int(n_blocks)),
               "nexrRingAllReduceSymmetricLL")

    def reduce_scatter_symmetric_ll(self, sendbuffs, recvbuffs, recvcount: int, datatype: int, op: int,
                                    n_blocks: int = 0) -> None:
        """ncclReduceScatter as the reference's symmetric LL kernel ReduceScatter_LL in ONE launch
        (nexrRingReduceScatterSymmetricLL): recvbuffs[r] receives chunk r folded from rank 0's input on (not
        from rank r's, as reduce_scatter_symmetric), in fp32 with one rounding. Rules as
        all_reduce_symmetric_ll."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingReduceScatterSymmetricLL(self._h, s, r, int(recvcount), int(datatype), int(op),
                                                        int(n_blocks)), "nexrRingReduceScatterSymmetricLL")

    def all_gather_symmetric_ll(self, sendbuffs, recvbuffs, sendcount: int, datatype: int, n_blocks: int = 0) -> None:
        """ncclAllGather as the reference's symmetric LL kernel AllGather_LL in ONE launch
        (nexrRingAllGatherSymmetricLL): a bit copy through the communicator's windows; the bytes are the ring's
        all-gather's. Rules as all_reduce_symmetric_ll, every datatype the ring's all-gather takes."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllGatherSymmetricLL(self._h, s, r, int(sendcount), int(datatype), int(n_blocks)),
               "nexrRingAllGatherSymmetricLL")

    def all_reduce_flat(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int) -> None:
        """The ring's ncclAllReduce as ONE launch with the ring's own bytes (nexrRingAllReduceFlat): the chain
        of one reduce-copy step per rank runs in registers, over this communicator's own chunks, user input
        first for SIMPLE and partial first for LL / LL128. Every datatype and op of all_reduce. Thread ranks,
        device memory, every rank on one GPU; or thread ranks in host memory with SIMPLE and the library's own
        reduce-copy, which run the host form (nexrFlatHostAllReduce: pinned buffers in place over the link,
        pageable ones staged; ``flat_host_stats()`` of the package reports how). Else InvalidUsage. Touches no
        connection: mixes with ring, tree and group calls, queued() stays as it was."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllReduceFlat(self._h, s, r, int(count), int(datatype), int(op)),
               "nexrRingAllReduceFlat")

    def reduce_scatter_flat(self, sendbuffs, recvbuffs, recvcount: int, datatype: int, op: int) -> None:
        """The ring's ncclReduceScatter as ONE launch with the ring's own bytes (nexrRingReduceScatterFlat):
        chunk d is folded from rank d + 1 on and ends at rank d. Rules as all_reduce_flat."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingReduceScatterFlat(self._h, s, r, int(recvcount), int(datatype), int(op)),
               "nexrRingReduceScatterFlat")

    def reduce_flat(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int, root: int) -> None:
        """The ring's ncclReduce as ONE launch with the ring's own bytes (nexrRingReduceFlat): the chain starts
        at root + 1 and ends at root; only recvbuffs[root] is needed and written. Rules as all_reduce_flat."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingReduceFlat(self._h, s, r, int(count), int(datatype), int(op), int(root)),
               "nexrRingReduceFlat")

    def tree_all_reduce_flat(self, sendbuffs, recvbuffs, count: int, datatype: int, op: int) -> None:
        """The tree's ncclAllReduce as ONE launch with the FIFO tree's own bytes (nexrTreeAllReduceFlat): every
        rank's one step over its own input and its children's values, interpreted in registers over this
        communicator's channel parts and every channel's own tree. Rules as all_reduce_flat."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrTreeAllReduceFlat(self._h, s, r, int(count), int(datatype), int(op)),
               "nexrTreeAllReduceFlat")

    def broadcast_flat(self, sendbuffs, recvbuffs, count: int, datatype: int, root: int) -> None:
        """ncclBroadcast as ONE launch (nexrRingBroadcastFlat): a bit copy of sendbuffs[root] to every recvbuff
        that is not that buffer itself; only the root's sendbuff is needed. Rules as all_reduce_flat."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingBroadcastFlat(self._h, s, r, int(count), int(datatype), int(root)),
               "nexrRingBroadcastFlat")

    def all_gather_flat(self, sendbuffs, recvbuffs, sendcount: int, datatype: int) -> None:
        """ncclAllGather as ONE launch (nexrRingAllGatherFlat): all_gather_symmetric under the flat name, whose
        bytes are the ring's."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        _check(self._L.nexrRingAllGatherFlat(self._h, s, r, int(sendcount), int(datatype)), "nexrRingAllGatherFlat")

    def set_flat(self, on: bool, tree: bool = False, copies: bool = False) -> None:
        """Opt in to (or out of) flat launches for the plain calls (nexrRingCommSetFlat). `on` (FLAT_RING):
        all_reduce, reduce_scatter and reduce; `tree` (FLAT_TREE): tree_all_reduce; `copies` (FLAT_COPIES):
        all_gather and broadcast. The chosen calls then run as their _flat forms where the communicator is
        eligible (thread ranks, device memory, one GPU, the library's own kernels; or thread ranks in host
        memory with SIMPLE and the library's own reduce-copy), with the same bytes, and queued() == 4 after such
        a call; every other call runs as without it. Between collectives; InvalidUsage for process-rank
        communicators and for host-memory communicators with a caller's fn, LL or LL128."""
        bits = (FLAT_RING if on else 0) | (FLAT_TREE if tree else 0) | (FLAT_COPIES if copies else 0)
        _check(self._L.nexrRingCommSetFlat(self._h, bits), "nexrRingCommSetFlat")

    def group_start(self) -> None:
        """ncclGroupStart (nexrRingGroupStart): the collectives of this communicator are recorded until the
        matching group_end. Nests by depth. InvalidUsage for process-rank communicators."""
        _check(self._L.nexrRingGroupStart(self._h), "nexrRingGroupStart")

    def group_end(self) -> None:
        """ncclGroupEnd (nexrRingGroupEnd): the outermost one runs the recorded calls, those that would run flat
        as flat group launches (one launch per kind between two conflicts, one wait), every other one alone at its
        place; the bytes are those of the calls made one by one. queued() == 5 after an end that queued a group
        launch. InvalidUsage without a group_start."""
        _check(self._L.nexrRingGroupEnd(self._h), "nexrRingGroupEnd")

    def group(self) -> "_Group":
        """``with comm.group(): ...``: group_start / group_end around the block."""
        return _Group(self)

    def group_stats(self, reset: bool = False) -> dict:
        """nexrRingGroupGetStats: calls recorded, group launches, fill launches, calls run singly and cuts since
        creation or the last reset."""
        st = RingGroupStats()
        _check(self._L.nexrRingGroupGetStats(self._h, ctypes.byref(st), 1 if reset else 0), "nexrRingGroupGetStats")
        return {"calls": st.calls, "group_launches": st.groupLaunches, "fill_launches": st.fillLaunches,
                "singles": st.singles, "cuts": st.cuts}

    def create_premul_sum(self, scalars, datatype: int, residence: int = SCALAR_HOST_IMMEDIATE) -> int:
        """ncclRedOpCreatePreMulSum for all ranks at once (nexrRingRedOpCreatePreMulSum): the handle of an op
        under which rank r's own input is multiplied by scalars[r] before the sum. SCALAR_HOST_IMMEDIATE:
        scalars[r] is one element of `datatype` as bytes or as anything with ``tobytes()`` (a numpy scalar of the
        datatype's width), copied now. SCALAR_DEVICE: scalars[r] is an address, kept and read during every
        collective that uses the op. None or a missing entry is passed on as a null pointer (InvalidArgument).
        The handle goes where all_reduce, reduce_scatter, reduce, tree_all_reduce and their _flat forms take an
        op; with differing scalars the group options and set_flat fall back (queued() reports what ran)."""
        if scalars is None:
            ptrs = None
        else:
            if len(scalars) != self.n_ranks:
                raise NexrError(Result.InvalidArgument, "one scalar per rank")
            keep = []
            ptrs = (ctypes.c_void_p * self.n_ranks)()
            for r, v in enumerate(scalars):
                if v is None:
                    ptrs[r] = None
                elif residence == SCALAR_HOST_IMMEDIATE:
                    raw = v.tobytes() if hasattr(v, "tobytes") else bytes(v)
                    keep.append(ctypes.create_string_buffer(raw + bytes(8), len(raw) + 8))
                    ptrs[r] = ctypes.addressof(keep[-1])
                else:
                    ptrs[r] = int(v)
        op = ctypes.c_int(-1)
        _check(self._L.nexrRingRedOpCreatePreMulSum(self._h, ctypes.byref(op), ptrs, int(datatype), int(residence)),
               "nexrRingRedOpCreatePreMulSum")
        return int(op.value)

    def destroy_op(self, op: int) -> None:
        """ncclRedOpDestroy (nexrRingRedOpDestroy): the handle is the next one create_premul_sum hands out.
        InvalidArgument for a built-in op and for a handle that is not live."""
        _check(self._L.nexrRingRedOpDestroy(self._h, int(op)), "nexrRingRedOpDestroy")

    def send_recv(self, sendbuffs, send_peers, recvbuffs, recv_peers, nbytes: int) -> None:
        """ncclSend/ncclRecv of every rank in one group: rank r sends nbytes of sendbuffs[r] to
        send_peers[r] and receives nbytes from recv_peers[r] into recvbuffs[r] (-1: none)."""
        s, r = self._arrays(sendbuffs, recvbuffs)
        sp = (ctypes.c_int * self.n_ranks)(*[int(v) for v in send_peers])
        rp = (ctypes.c_int * self.n_ranks)(*[int(v) for v in recv_peers])
        _check(self._extras().nexrSendRecv(self._h, s, sp, r, rp, int(nbytes)), "nexrSendRecv")

    def step_wait(self) -> str:
        """"word" or "sync": how this communicator's rank threads wait for a device step
        (nexrRingCommGetStepWait; sync when the ranks span GPUs)."""
        w = ctypes.c_int()
        _check(self._L.nexrRingCommGetStepWait(self._h, ctypes.byref(w)), "nexrRingCommGetStepWait")
        return "word" if w.value else "sync"

    def queued(self) -> int:
        """How the last ring collective ran its LL steps (nexrRingCommGetQueued): 5 flat group launches (a
        group_end that queued at least one), 4 one flat launch (set_flat),
        3 group launches on
        one stream (set_ll_group; set_simple_group for SIMPLE), 2 runs on the device with device credits, 1 queued launches,
        0 host-sequenced (LL steps need every rank on one GPU and device memory for 1, 2 or 3; 1 and 2
        also a hardware queue per rank stream). While set_ll_group is on, a tree_all_reduce reports here
        too: 3 when it ran as group launches, 0 when it fell back."""
        w = ctypes.c_int()
        _check(self._L.nexrRingCommGetQueued(self._h, ctypes.byref(w)), "nexrRingCommGetQueued")
        return int(w.value)

    def set_ll_group(self, on: bool) -> None:
        """Opt in to (or out of) group launches (nexrRingCommSetLLGroup): the LL steps of every rank and
        channel of a ring collective in the same launches on one stream, queued() == 3. LL128
        communicators too (nexrReduceCopyLL128StepsGroup, the ordered hand-off); without the option they
        stay host-sequenced. Between collectives; InvalidUsage unless the communicator is thread-rank, LL
        or LL128, and device-memory.

        tree_all_reduce takes the option too: the root and every other rank's reduce-up and broadcast-down
        halves are the members, 2n - 1 per channel, and queued() is 3 after it. It falls back to
        host-sequenced steps (queued() == 0) when the ranks span GPUs, with a caller's ll_fn / ll128_fn,
        above 32 members over all channels, or when the grid is not resident at once. With the option off
        a tree call leaves queued() as it was."""
        _check(self._L.nexrRingCommSetLLGroup(self._h, 1 if on else 0), "nexrRingCommSetLLGroup")

    def set_simple_group(self, on: bool) -> None:
        """Opt in to (or out of) SIMPLE group launches (nexrRingCommSetSimpleGroup): the slices of every rank
        and channel of a ring collective as step lists in the same launches on one stream
        (nexrReduceCopySimpleStepsGroup), tails and heads in device memory, queued() == 3. Between
        collectives; InvalidUsage unless the communicator is thread-rank, SIMPLE and device-memory. A
        collective falls back to host-sequenced steps (queued() == 0) when the ranks span GPUs, with a
        caller's fn, the hipStreamSynchronize step wait, more than 32 members, or a grid that is not resident
        at once even at one workgroup per member. tree_all_reduce does not take it."""
        _check(self._L.nexrRingCommSetSimpleGroup(self._h, 1 if on else 0), "nexrRingCommSetSimpleGroup")

    def set_direct(self, on: bool) -> None:
        """State that the user buffers of the following ring collectives are registered
        (nexrRingCommSetDirect): SIMPLE senders then write into the next rank's recvbuff instead of a FIFO
        slot (DirectWrite) in AllGather, Broadcast and out-of-place AllReduce; every other call runs as
        without it. Between collectives; InvalidUsage unless the communicator is thread-rank and SIMPLE.
        Combines with set_simple_group."""
        _check(self._L.nexrRingCommSetDirect(self._h, 1 if on else 0), "nexrRingCommSetDirect")

    def direct_slices(self) -> tuple:
        """(direct, fifo): the last ring collective's send slices of either kind over all ranks and channels
        (nexrRingCommGetDirect)."""
        d, f = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.nexrRingCommGetDirect(self._h, ctypes.byref(d), ctypes.byref(f)), "nexrRingCommGetDirect")
        return int(d.value), int(f.value)

    def set_ll_flag_rule(self, flag_max: int, clean_mask: int) -> None:
        """The LL flag rule of every channel (nexrRingCommSetLLFlagRule): (0, 0x7ffffff8) is the production
        rule, (0x100, 0x78) the reference's TEST_LL_CLEANUP. Only before the first collective."""
        rule = LLFlagRule(int(flag_max), int(clean_mask))
        _check(self._L.nexrRingCommSetLLFlagRule(self._h, ctypes.byref(rule)), "nexrRingCommSetLLFlagRule")

    def ll_cleanup(self):
        """(min_send_step, cleaned_steps) (nexrRingCommGetLLCleanup): the smallest send-step counter among
        the connections that have sent, and the cleaning send steps run since creation."""
        lo, cleaned = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.nexrRingCommGetLLCleanup(self._h, ctypes.byref(lo), ctypes.byref(cleaned)),
               "nexrRingCommGetLLCleanup")
        return int(lo.value), int(cleaned.value)

    def tree_topology(self, rank: int):
        """(up, [down...]) of `rank` in this communicator's tree (-1 = none)."""
        up = ctypes.c_int()
        down = (ctypes.c_int * 3)()
        _check(self._L.nexrTreeTopology(self._h, int(rank), ctypes.byref(up), down), "nexrTreeTopology")
        return up.value, [d for d in down if d >= 0]

    def _extras(self) -> ctypes.CDLL:
        if not self.extras:
            raise NexrError(Result.InvalidUsage, "send/recv and the resident collectives are in the opt-in extras "
                                                 "library: create the communicator with extras=True")
        return self._L

    def close(self) -> None:
        if self._h:
            self._L.nexrRingCommDestroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PeerRingComm:
    """This process's rank of a ring whose ranks are processes (one per GPU), FIFOs shared over IPC.

    Every rank passes the same fresh ``shm_name`` (e.g. made by rank 0 and broadcast out of band);
    the constructor blocks until all ``n_ranks`` processes have joined."""

    def __init__(self, n_ranks: int, rank: int, shm_name: str, device: int = 0, buff_bytes: int = 0,
                 protocol: int = PROTO_SIMPLE, timeout_ms: int = 0, extras: bool = False):
        self._name = shm_name.encode()
        cfg = PeerRingConfig(n_ranks, rank, device, buff_bytes, protocol, timeout_ms, self._name)
        self._L = extras_lib() if extras else ring_lib()
        self.extras = extras
        h = ctypes.c_void_p()
        _check(self._L.nexrPeerRingCommCreate(ctypes.byref(h), ctypes.byref(cfg)), "nexrPeerRingCommCreate")
        self._h = h
        self.n_ranks, self.rank = n_ranks, rank

    def all_reduce(self, sendbuff: int, recvbuff: int, count: int, datatype: int, op: int) -> None:
        _check(self._L.nexrPeerRingAllReduce(self._h, int(sendbuff) or None, int(recvbuff) or None, int(count),
                                                int(datatype), int(op)), "nexrPeerRingAllReduce")

    def all_reduce_resident(self, sendbuff: int, recvbuff: int, count: int, datatype: int, op: int) -> None:
        """This rank's part of the all-reduce as one device-resident launch (nexrPeerRingAllReduceResident)."""
        _check(self._extras().nexrPeerRingAllReduceResident(self._h, int(sendbuff) or None, int(recvbuff) or None,
                                                        int(count), int(datatype), int(op)),
               "nexrPeerRingAllReduceResident")

    def reduce_scatter(self, sendbuff: int, recvbuff: int, recvcount: int, datatype: int, op: int) -> None:
        _check(self._L.nexrPeerRingReduceScatter(self._h, int(sendbuff) or None, int(recvbuff) or None,
                                                    int(recvcount), int(datatype), int(op)), "nexrPeerRingReduceScatter")

    def all_gather(self, sendbuff: int, recvbuff: int, sendcount: int, datatype: int) -> None:
        _check(self._L.nexrPeerRingAllGather(self._h, int(sendbuff) or None, int(recvbuff) or None, int(sendcount),
                                                int(datatype)), "nexrPeerRingAllGather")

    def reduce(self, sendbuff: int, recvbuff: int, count: int, datatype: int, op: int, root: int) -> None:
        _check(self._L.nexrPeerRingReduce(self._h, int(sendbuff) or None, int(recvbuff) or None, int(count),
                                             int(datatype), int(op), int(root)), "nexrPeerRingReduce")

    def send_recv(self, sendbuff: int, send_peer: int, recvbuff: int, recv_peer: int, nbytes: int) -> None:
        _check(self._extras().nexrPeerSendRecv(self._h, int(sendbuff) or None, int(send_peer), int(recvbuff) or None,
                                           int(recv_peer), int(nbytes)), "nexrPeerSendRecv")

    def step_wait(self) -> str:
        """"word" or "sync": how this communicator's rank threads wait for a device step
        (nexrRingCommGetStepWait; sync when the ranks span GPUs)."""
        w = ctypes.c_int()
        _check(self._L.nexrRingCommGetStepWait(self._h, ctypes.byref(w)), "nexrRingCommGetStepWait")
        return "word" if w.value else "sync"

    def broadcast(self, sendbuff: int, recvbuff: int, count: int, datatype: int, root: int) -> None:
        _check(self._L.nexrPeerRingBroadcast(self._h, int(sendbuff) or None, int(recvbuff) or None, int(count),
                                                int(datatype), int(root)), "nexrPeerRingBroadcast")

    def _extras(self) -> ctypes.CDLL:
        if not self.extras:
            raise NexrError(Result.InvalidUsage, "send/recv and the resident collectives are in the opt-in extras "
                                                 "library: create the communicator with extras=True")
        return self._L

    def close(self) -> None:
        if self._h:
            self._L.nexrRingCommDestroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
