"""nex-nccl_amd — MI355X-native reduce-copy primitive (host-side mirror of the reference API).

The product is ``libnexr.so`` (C ABI, ``include/nexr.h``) built from ``csrc/`` for gfx950. This
module is the Python view of that boundary, mirroring the reference's operator interface for the
path: the device primitive ``reduceCopy`` (src/device/common_kernel.h:331-349), the one-rank
launcher ``ncclLaunchOneRank`` (src/device/onerank.cc:48-83) and the op encoder
``hostToDevRedOp`` (src/enqueue.cc:2185-2278). Same argument meaning, same integer enums and
result codes; failures raise :class:`NexrError` carrying the ``ncclResult_t``-compatible code.

There is no fallback: if ``libnexr.so`` is missing or fails to load, every call raises.
Import it with ``importlib.import_module("nex-nccl_amd")`` (the directory name has a hyphen).
"""
from __future__ import annotations

import ctypes
import enum
import os
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnexr.so")

MAX_SRCS = 8
MAX_DSTS = 8


class Result(enum.IntEnum):
    """ncclResult_t values (reference src/nccl.h.in:40-48)."""
    Success = 0
    UnhandledCudaError = 1
    SystemError = 2
    InternalError = 3
    InvalidArgument = 4
    InvalidUsage = 5
    RemoteError = 6
    InProgress = 7


class DataType(enum.IntEnum):
    """ncclDataType_t values (reference src/nccl.h.in:278-290)."""
    Int8 = 0
    Uint8 = 1
    Int32 = 2
    Uint32 = 3
    Int64 = 4
    Uint64 = 5
    Float16 = 6
    Float32 = 7
    Float64 = 8
    Bfloat16 = 9
    Float8e4m3 = 10
    Float8e5m2 = 11


class RedOp(enum.IntEnum):
    """ncclRedOp_t built-in values (reference src/nccl.h.in:259-270)."""
    Sum = 0
    Prod = 1
    Max = 2
    Min = 3
    Avg = 4


class DevRedOp(enum.IntEnum):
    """ncclDevRedOp_t values (reference src/include/device.h:683-687)."""
    Sum = 0
    Prod = 1
    MinMax = 2
    PreMulSum = 3
    SumPostDiv = 4


class Semantics(enum.IntEnum):
    """nexrSemantics_t (include/nexr.h): which nex-nccl the library reproduces bit for bit."""
    Nccl = 0     # real arithmetic, min/max at the datatype's signedness (default)
    Fork = 1     # the fork with SKIP_COMP removed: signed min/max on the unsigned kernel (generate.py:128-136)
    Shipped = 2  # the fork as shipped: SKIP_COMP (reduce_kernel.h:432), every reduce returns its first operand


TYPE_SIZE = {DataType.Int8: 1, DataType.Uint8: 1, DataType.Int32: 4, DataType.Uint32: 4,
             DataType.Int64: 8, DataType.Uint64: 8, DataType.Float16: 2, DataType.Float32: 4,
             DataType.Float64: 8, DataType.Bfloat16: 2, DataType.Float8e4m3: 1,
             DataType.Float8e5m2: 1}

# ABI symbols declared in include/nexr.h (checked by tests/test_abi.py)
ABI_SYMBOLS = ("nexrReduceCopy", "nexrReduceCopyBatch", "nexrReduceCopyMultiDevice", "nexrReduceCopyMultiDeviceSets",
               "nexrReduceCopyHost", "nexrHostToDevRedOp", "nexrLaunchOneRank",
               "nexrReduceCopyLL", "nexrReduceCopyLL128", "nexrReduceCopyLLSteps", "nexrReduceCopyLLStepsRule",
               "nexrLLGroupWorkspaceBytes", "nexrReduceCopyLLStepsGroup", "nexrReduceCopyLL128StepsGroup",
               "nexrSimpleGroupWorkspaceBytes", "nexrReduceCopySimpleStepsGroup",
               "nexrSimpleGroupDirectWorkspaceBytes", "nexrReduceCopySimpleStepsGroupDirect", "nexrSymAllReduce",
               "nexrSymReduceScatter", "nexrSymAllGather", "nexrSymLLWindowBytes", "nexrSymLLAllReduce",
               "nexrSymLLReduceScatter", "nexrSymLLAllGather",
               "nexrFlatAllReduce", "nexrFlatReduceScatter", "nexrFlatReduce",
               "nexrFlatTreeAllReduce", "nexrFlatBroadcast",
               "nexrFlatAllReducePreMul", "nexrFlatReduceScatterPreMul", "nexrFlatReducePreMul",
               "nexrFlatTreeAllReducePreMul",
               "nexrFlatHostAllReduce", "nexrFlatHostReduceScatter", "nexrFlatHostReduce",
               "nexrFlatHostTreeAllReduce", "nexrFlatHostBroadcast", "nexrFlatHostAllGather", "nexrGetFlatHostStats",
               "nexrFlatGroup", "nexrFlatGroupPlan",
               "nexrLLCleanSlot", "nexrQueryLaunch", "nexrGetPoolStats", "nexrTypeSize", "nexrGetErrorString", "nexrGetVersion",
               "nexrGetLastHipError", "nexrSetSemantics", "nexrGetSemantics", "nexrHostRegister", "nexrHostDeregister",
               "nexrHostMemAlloc", "nexrHostMemFree", "nexrGetHostPathStats")


class NexrError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = int(code)
        try:
            name = Result(self.code).name
        except ValueError:
            name = "Unknown"
        super().__init__(f"{what}: nexr result {self.code} ({name})" if what else f"nexr result {self.code} ({name})")


class FlatPart(ctypes.Structure):
    """nexrFlatPart: one channel's part of a flat all-reduce, in elements."""
    _fields_ = [("offset", ctypes.c_uint64), ("count", ctypes.c_uint64), ("chunkCount", ctypes.c_uint64)]


class FlatGroupWork(ctypes.Structure):
    """nexrFlatGroupWork: one call of a flat group (include/nexr.h)."""
    _fields_ = [("coll", ctypes.c_int), ("datatype", ctypes.c_int), ("devRedOp", ctypes.c_int), ("root", ctypes.c_int),
                ("redOpArg", ctypes.c_uint64), ("inputs", ctypes.POINTER(ctypes.c_void_p)),
                ("outputs", ctypes.POINTER(ctypes.c_void_p)), ("nOutputs", ctypes.c_int), ("nParts", ctypes.c_int),
                ("parts", ctypes.POINTER(FlatPart)), ("nElts", ctypes.c_size_t)]


class FlatGroupInfo(ctypes.Structure):
    """nexrFlatGroupInfo: what a flat group call made of its works."""
    _fields_ = [("works", ctypes.c_int), ("launches", ctypes.c_int), ("fillLaunches", ctypes.c_int),
                ("cuts", ctypes.c_int), ("tableBytes", ctypes.c_uint64), ("workgroups", ctypes.c_uint64)]


class FlatTreeLinks(ctypes.Structure):
    """nexrFlatTreeLinks: one rank's links in a tree, -1 for none, children packed first."""
    _fields_ = [("up", ctypes.c_int), ("down", ctypes.c_int * 3)]


class FlatTreePart(ctypes.Structure):
    """nexrFlatTreePart: one channel's part of a flat tree all-reduce, in elements, and its tree's index."""
    _fields_ = [("offset", ctypes.c_uint64), ("count", ctypes.c_uint64), ("tree", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class DevRedOpFull(ctypes.Structure):
    """Byte-exact mirror of struct ncclDevRedOpFull (reference src/include/device.h:688-693): enum op
    at 0, enum proxyOp at 4, bool scalarArgIsPtr at 8 (9-15 padding), uint64 scalarArg at 16."""
    _fields_ = [("op", ctypes.c_int), ("proxyOp", ctypes.c_int), ("scalarArgIsPtr", ctypes.c_bool),
                ("scalarArg", ctypes.c_uint64)]


class LaunchInfo(ctypes.Structure):
    """Mirror of nexrLaunchInfo (include/nexr.h): what nexrQueryLaunch reports."""
    _fields_ = [("grid", ctypes.c_uint32), ("block", ctypes.c_int), ("packsPerLane", ctypes.c_int),
                ("policy", ctypes.c_int), ("unaligned", ctypes.c_int),
                ("headElts", ctypes.c_uint64),
                ("bodyPacks", ctypes.c_uint64)]


class HostPathStats(ctypes.Structure):
    """Mirror of nexrHostPathStats (include/nexr.h): nexrGetHostPathStats' counters."""
    _fields_ = [(f, ctypes.c_uint64) for f in ("calls", "zeroCopyCalls", "registeredHits", "pointerQueries",
                                               "classifyNs", "copyNs", "launchNs", "waitNs")]


class FlatHostStats(ctypes.Structure):
    """Mirror of nexrFlatHostStats (include/nexr.h): nexrGetFlatHostStats' counters."""
    _fields_ = [(f, ctypes.c_uint64) for f in ("calls", "zeroCopyCalls", "stagedBuffers", "registeredHits",
                                               "pointerQueries", "windows")]


MAX_BATCH_WORKS = 14  # NEXR_MAX_BATCH_WORKS


class ReduceCopyWork(ctypes.Structure):
    """Mirror of nexrReduceCopyWork (include/nexr.h): one reduce-copy of a batch."""
    _fields_ = [("nSrcs", ctypes.c_int), ("nDsts", ctypes.c_int), ("srcs", ctypes.c_void_p * 8),
                ("dsts", ctypes.c_void_p * 8), ("nElts", ctypes.c_size_t), ("redOpArg", ctypes.c_uint64),
                ("nPreOpSrcs", ctypes.c_int), ("postOp", ctypes.c_int), ("preOpArgs", ctypes.c_uint64 * 8)]


LL_STEPS_MAX_PEERS = 3  # NEXR_LL_STEPS_MAX_PEERS
LL_HEAD_BYTES = 4096   # NEXR_LL_HEAD_BYTES
LL_GROUP_MAX_MEMBERS = 32  # NEXR_LL_GROUP_MAX_MEMBERS
LL_GROUP_LAUNCHES = 8      # NEXR_LL_GROUP_LAUNCHES: the launches nexrLLGroupWorkspaceBytes sizes for


class LLStep(ctypes.Structure):
    """Mirror of nexrLLStep (include/nexr.h): one LLGenericOp call of a run (32 bytes)."""
    _fields_ = [("srcIx", ctypes.c_int64), ("dstIx", ctypes.c_int64), ("nElts", ctypes.c_uint32),
                ("recv", ctypes.c_uint8), ("send", ctypes.c_uint8), ("srcBuf", ctypes.c_int8),
                ("dstBuf", ctypes.c_int8), ("postOp", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 7)]


class LLConnSet(ctypes.Structure):
    """Mirror of nexrLLConnSet (include/nexr.h): the connections a run of LL steps uses."""
    _fields_ = [("input", ctypes.c_void_p), ("output", ctypes.c_void_p), ("nRecv", ctypes.c_int),
                ("nSend", ctypes.c_int), ("recvFifo", ctypes.c_void_p * 3), ("recvHead", ctypes.c_void_p * 3),
                ("recvStep", ctypes.c_uint64 * 3), ("sendFifo", ctypes.c_void_p * 3),
                ("sendHead", ctypes.c_void_p * 3), ("sendStep", ctypes.c_uint64 * 3),
                ("slotBytes", ctypes.c_uint64), ("nSlots", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


SIMPLE_CREDIT_BYTES = 4096   # NEXR_SIMPLE_CREDIT_BYTES: a connection's tail block, and its head block
SIMPLE_GROUP_MAX_GRID = 256  # NEXR_SIMPLE_GROUP_MAX_GRID
SIMPLE_TILE_BYTES = 4096     # tile t of a slice belongs to workgroup t % G


class SimpleConnSet(ctypes.Structure):
    """Mirror of nexrSimpleConnSet (include/nexr.h): the connections a SIMPLE step list uses."""
    _fields_ = [("input", ctypes.c_void_p), ("output", ctypes.c_void_p), ("nRecv", ctypes.c_int),
                ("nSend", ctypes.c_int), ("recvFifo", ctypes.c_void_p * 3), ("recvTail", ctypes.c_void_p * 3),
                ("recvHead", ctypes.c_void_p * 3), ("recvStep", ctypes.c_uint64 * 3),
                ("sendFifo", ctypes.c_void_p * 3), ("sendTail", ctypes.c_void_p * 3),
                ("sendHead", ctypes.c_void_p * 3), ("sendStep", ctypes.c_uint64 * 3),
                ("slotBytes", ctypes.c_uint64), ("nSlots", ctypes.c_uint32), ("stepPerSlice", ctypes.c_uint32)]


SIMPLE_DIRECT_RECV = 1  # NEXR_SIMPLE_DIRECT_RECV: LLStep.pad[0] bit, DirectRecv1 of genericOp
SIMPLE_DIRECT_SEND = 2  # NEXR_SIMPLE_DIRECT_SEND: DirectSend1


class SimpleDirectSet(ctypes.Structure):
    """Mirror of nexrSimpleDirectSet (include/nexr.h): a member's direct ends (32 bytes)."""
    _fields_ = [("sendDirect", ctypes.c_void_p * 3), ("recvDirect", ctypes.c_uint8 * 3), ("pad", ctypes.c_uint8 * 5)]


class LLFlagRule(ctypes.Structure):
    """Mirror of nexrLLFlagRule (include/nexr.h): flagMax 0 means NCCL_LL_FLAG(a) = (uint32_t)a, else
    a % flagMax; a send step s cleans its slot when (s & cleanMask) == cleanMask."""
    _fields_ = [("flagMax", ctypes.c_uint32), ("cleanMask", ctypes.c_uint32)]


LL_PRODUCTION_RULE = (0, 0x7FFFFFF8)  # NCCL_LL_CLEAN_MASK with 32-bit flags
LL_TEST_RULE = (0x100, 0x78)          # the reference's TEST_LL_CLEANUP (src/include/device.h:719-728)


def _ll_rule(rule) -> LLFlagRule:
    """An LLFlagRule from None (the production rule), an LLFlagRule or a (flag_max, clean_mask) pair."""
    if rule is None:
        rule = LL_PRODUCTION_RULE
    if isinstance(rule, LLFlagRule):
        return rule
    flag_max, clean_mask = rule
    return LLFlagRule(int(flag_max), int(clean_mask))


def ll_flag(step: int, rule=None) -> int:
    """The flag the lines of step `step` carry: NCCL_LL_FLAG(step + 1) under the rule."""
    r = _ll_rule(rule)
    a = int(step) + 1
    return a % r.flagMax if r.flagMax else a & 0xFFFFFFFF


def ll_cleans(step: int, rule=None) -> bool:
    """Whether send step `step` cleans its slot: (step & cleanMask) == cleanMask (incSend, prims_ll.h:85-93)."""
    r = _ll_rule(rule)
    return (int(step) & r.cleanMask) == r.cleanMask


_lib = None


def hip_runtime() -> ctypes.CDLL:
    """The HIP runtime libnexr runs on (the one libamdhip64 mapped in this process, see lib()), for
    harness calls the ABI does not cover (hipDeviceEnablePeerAccess in tools/xgmi_probe.py)."""
    lib()
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln and "/" in ln})
    if len(paths) != 1:
        raise NexrError(Result.InternalError, f"expected one HIP runtime in the process, found {paths}")
    return ctypes.CDLL(paths[0])


def _preload_hip_runtime() -> None:
    """One HIP runtime per process. torch ships its own libamdhip64 (soname libamdhip64.so.7, NEEDED
    by torch as "libamdhip64.so" through its RUNPATH), so loading libnexr first would map
    /opt/rocm's runtime and torch then a second one: torch's streams and allocations would be
    foreign handles to libnexr (hipErrorNoDevice / invalid handle at the first launch). When a
    runtime is already mapped (torch imported, or any other), libnexr's NEEDED libamdhip64.so.7
    resolves to it. Otherwise, if torch is installed, its runtime file is mapped here by path,
    without importing torch: libnexr then binds to it through the soname, and a later `import
    torch` finds that same file already mapped. Without torch, /opt/rocm's runtime serves."""
    with open("/proc/self/maps") as f:
        if any("libamdhip64" in ln for ln in f):
            return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        cand = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            return


def lib() -> ctypes.CDLL:
    """Load libnexr.so (raises if it is missing: there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NexrError(Result.InternalError,
                        f"{LIB_PATH} not built (run __graft_entry__.build() or make -C nex-nccl_amd/csrc)")
    _preload_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, i32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    P = ctypes.POINTER
    for name in ("nexrReduceCopy", "nexrReduceCopyHost"):
        f = getattr(L, name)
        f.argtypes = [i32, P(vp), i32, P(vp), sz, i32, i32, u64, i32, P(u64), i32, vp]
        f.restype = i32
    L.nexrReduceCopyBatch.argtypes = [P(ReduceCopyWork), i32, i32, i32, vp]
    L.nexrReduceCopyBatch.restype = i32
    L.nexrReduceCopyMultiDevice.argtypes = [P(ReduceCopyWork), P(i32), i32, i32, i32, i32, P(ctypes.c_double)]
    L.nexrReduceCopyMultiDevice.restype = i32
    L.nexrReduceCopyMultiDeviceSets.argtypes = [P(ReduceCopyWork), P(i32), i32, i32, i32, i32, i32, P(ctypes.c_double)]
    L.nexrReduceCopyMultiDeviceSets.restype = i32
    L.nexrHostToDevRedOp.argtypes = [P(DevRedOpFull), i32, i32, i32]
    L.nexrHostToDevRedOp.restype = i32
    L.nexrLaunchOneRank.argtypes = [vp, vp, sz, DevRedOpFull, i32, vp]
    L.nexrLaunchOneRank.restype = i32
    L.nexrQueryLaunch.argtypes = [i32, P(vp), i32, P(vp), sz, i32, P(LaunchInfo)]
    L.nexrQueryLaunch.restype = i32
    L.nexrGetPoolStats.argtypes = [P(u64), P(u64)]
    L.nexrGetPoolStats.restype = i32
    L.nexrSetSemantics.argtypes = [i32]
    L.nexrSetSemantics.restype = i32
    L.nexrGetSemantics.argtypes = [P(i32)]
    L.nexrGetSemantics.restype = i32
    L.nexrReduceCopyLL.argtypes = [vp, i32, i32, P(vp), P(ctypes.c_uint32), vp, i32, P(vp), P(ctypes.c_uint32), sz,
                                   i32, i32, u64, i32, vp, ctypes.c_uint32, vp]
    L.nexrReduceCopyLL.restype = i32
    L.nexrReduceCopyLL128.argtypes = [vp, i32, i32, P(vp), P(u64), vp, i32, P(vp), P(u64), sz,
                                      i32, i32, u64, i32, vp, ctypes.c_uint32, vp]
    L.nexrReduceCopyLL128.restype = i32
    L.nexrReduceCopyLLSteps.argtypes = [P(LLConnSet), P(LLStep), i32, i32, i32, u64, vp, ctypes.c_uint32, vp]
    L.nexrReduceCopyLLSteps.restype = i32
    L.nexrReduceCopyLLStepsRule.argtypes = [P(LLConnSet), P(LLStep), i32, i32, i32, u64, P(LLFlagRule), vp,
                                            ctypes.c_uint32, vp]
    L.nexrReduceCopyLLStepsRule.restype = i32
    L.nexrLLGroupWorkspaceBytes.argtypes = [i32, P(sz)]
    L.nexrLLGroupWorkspaceBytes.restype = i32
    L.nexrReduceCopyLLStepsGroup.argtypes = [i32, P(LLConnSet), P(P(LLStep)), P(i32), i32, i32, u64, P(LLFlagRule),
                                             vp, ctypes.c_uint32, vp, sz, vp]
    L.nexrReduceCopyLLStepsGroup.restype = i32
    L.nexrReduceCopyLL128StepsGroup.argtypes = [i32, P(LLConnSet), P(P(LLStep)), P(i32), i32, i32, u64, vp,
                                                ctypes.c_uint32, vp, sz, vp]
    L.nexrReduceCopyLL128StepsGroup.restype = i32
    L.nexrSimpleGroupWorkspaceBytes.argtypes = [i32, P(sz)]
    L.nexrSimpleGroupWorkspaceBytes.restype = i32
    L.nexrReduceCopySimpleStepsGroup.argtypes = [i32, P(SimpleConnSet), P(P(LLStep)), P(i32), i32, i32, u64, i32, vp,
                                                 ctypes.c_uint32, vp, sz, vp]
    L.nexrReduceCopySimpleStepsGroup.restype = i32
    L.nexrSimpleGroupDirectWorkspaceBytes.argtypes = [i32, P(sz)]
    L.nexrSimpleGroupDirectWorkspaceBytes.restype = i32
    L.nexrReduceCopySimpleStepsGroupDirect.argtypes = [i32, P(SimpleConnSet), P(P(LLStep)), P(i32), i32, i32, u64, i32,
                                                       P(SimpleDirectSet), vp, ctypes.c_uint32, vp, sz, vp]
    L.nexrReduceCopySimpleStepsGroupDirect.restype = i32
    L.nexrSymAllReduce.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, i32, vp]
    L.nexrSymAllReduce.restype = i32
    L.nexrSymReduceScatter.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, vp]
    L.nexrSymReduceScatter.restype = i32
    L.nexrSymAllGather.argtypes = [i32, P(vp), P(vp), sz, vp]
    L.nexrSymAllGather.restype = i32
    L.nexrFlatAllReduce.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, i32, P(FlatPart), i32, vp]
    L.nexrFlatAllReduce.restype = i32
    L.nexrFlatReduceScatter.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, i32, vp]
    L.nexrFlatReduceScatter.restype = i32
    L.nexrFlatReduce.argtypes = [i32, P(vp), vp, i32, sz, i32, i32, u64, i32, vp]
    L.nexrFlatReduce.restype = i32
    L.nexrFlatTreeAllReduce.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, i32, P(P(FlatTreeLinks)), i32,
                                        P(FlatTreePart), i32, vp]
    L.nexrFlatTreeAllReduce.restype = i32
    L.nexrFlatBroadcast.argtypes = [i32, vp, P(vp), sz, vp]
    L.nexrFlatBroadcast.restype = i32
    L.nexrFlatAllReducePreMul.argtypes = [i32, P(vp), P(vp), sz, i32, P(u64), i32, i32, P(FlatPart), i32, vp]
    L.nexrFlatReduceScatterPreMul.argtypes = [i32, P(vp), P(vp), sz, i32, P(u64), i32, i32, vp]
    L.nexrFlatReducePreMul.argtypes = [i32, P(vp), vp, i32, sz, i32, P(u64), i32, i32, vp]
    L.nexrFlatTreeAllReducePreMul.argtypes = [i32, P(vp), P(vp), sz, i32, P(u64), i32, i32, P(P(FlatTreeLinks)), i32,
                                              P(FlatTreePart), i32, vp]
    for name in ("nexrFlatAllReducePreMul", "nexrFlatReduceScatterPreMul", "nexrFlatReducePreMul",
                 "nexrFlatTreeAllReducePreMul"):
        getattr(L, name).restype = i32
    for host, dev in (("nexrFlatHostAllReduce", L.nexrFlatAllReduce),
                      ("nexrFlatHostReduceScatter", L.nexrFlatReduceScatter), ("nexrFlatHostReduce", L.nexrFlatReduce),
                      ("nexrFlatHostTreeAllReduce", L.nexrFlatTreeAllReduce),
                      ("nexrFlatHostBroadcast", L.nexrFlatBroadcast), ("nexrFlatHostAllGather", L.nexrSymAllGather)):
        f = getattr(L, host)   # the device entry's argument list
        f.argtypes = dev.argtypes
        f.restype = i32
    L.nexrFlatGroup.argtypes = [i32, P(FlatGroupWork), i32, i32, i32, P(i32), P(FlatGroupInfo), vp]
    L.nexrFlatGroup.restype = i32
    L.nexrFlatGroupPlan.argtypes = [i32, P(FlatGroupWork), i32, i32, i32, P(i32), P(FlatGroupInfo)]
    L.nexrFlatGroupPlan.restype = i32
    L.nexrGetFlatHostStats.argtypes = [P(FlatHostStats), i32]
    L.nexrGetFlatHostStats.restype = i32
    L.nexrSymLLWindowBytes.argtypes = [i32, i32, P(sz)]
    L.nexrSymLLWindowBytes.restype = i32
    L.nexrSymLLAllReduce.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, P(vp), sz, i32, vp, ctypes.c_uint32, vp]
    L.nexrSymLLAllReduce.restype = i32
    L.nexrSymLLReduceScatter.argtypes = [i32, P(vp), P(vp), sz, i32, i32, u64, P(vp), sz, i32, vp, ctypes.c_uint32,
                                         vp]
    L.nexrSymLLReduceScatter.restype = i32
    L.nexrSymLLAllGather.argtypes = [i32, P(vp), P(vp), sz, P(vp), sz, i32, vp, ctypes.c_uint32, vp]
    L.nexrSymLLAllGather.restype = i32
    L.nexrLLCleanSlot.argtypes = [i32, P(vp), P(ctypes.c_uint32), sz, sz, vp]
    L.nexrLLCleanSlot.restype = i32
    L.nexrTypeSize.argtypes = [i32]
    L.nexrTypeSize.restype = sz
    L.nexrGetErrorString.argtypes = [i32]
    L.nexrGetErrorString.restype = ctypes.c_char_p
    L.nexrGetVersion.argtypes = []
    L.nexrGetVersion.restype = i32
    L.nexrGetLastHipError.argtypes = []
    L.nexrGetLastHipError.restype = i32
    L.nexrHostRegister.argtypes = [vp, sz, P(vp)]
    L.nexrHostRegister.restype = i32
    L.nexrHostDeregister.argtypes = [vp]
    L.nexrHostDeregister.restype = i32
    L.nexrHostMemAlloc.argtypes = [P(vp), sz]
    L.nexrHostMemAlloc.restype = i32
    L.nexrHostMemFree.argtypes = [vp]
    L.nexrHostMemFree.restype = i32
    L.nexrGetHostPathStats.argtypes = [P(HostPathStats), i32]
    L.nexrGetHostPathStats.restype = i32
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        extra = ""
        if rc == Result.UnhandledCudaError:
            extra = f" (hipError {lib().nexrGetLastHipError()})"
        raise NexrError(rc, what + extra)


def _ptr_array(ptrs: Sequence[int]):
    arr = (ctypes.c_void_p * max(1, len(ptrs)))()
    for i, p in enumerate(ptrs):
        arr[i] = ctypes.c_void_p(int(p)) if p else None
    return arr


def _u64_array(vals: Optional[Sequence[int]]):
    if not vals:
        return None
    arr = (ctypes.c_uint64 * len(vals))()
    for i, v in enumerate(vals):
        arr[i] = int(v) & 0xFFFFFFFFFFFFFFFF
    return arr


def reduce_copy_ptrs(srcs: Sequence[int], dsts: Sequence[int], n_elts: int, datatype: int, dev_red_op: int,
                     red_op_arg: int = 0, pre_op_args: Optional[Sequence[int]] = None, post_op: bool = False,
                     stream: int = 0, host: bool = False) -> None:
    """Raw-pointer reduce-copy through the C ABI (``nexrReduceCopy`` / ``nexrReduceCopyHost``).

    ``srcs``/``dsts`` are device addresses (host addresses when ``host=True``); ``stream`` is a
    hipStream_t handle (0 = default stream). Mirrors reduceCopy(…, redArg, preOpArgs, postOp,
    nSrcs, srcPtrs, nDsts, dstPtrs, nElts) (common_kernel.h:331-349)."""
    L = lib()
    pre = list(pre_op_args) if pre_op_args else []
    f = L.nexrReduceCopyHost if host else L.nexrReduceCopy
    rc = f(len(srcs), _ptr_array(srcs), len(dsts), _ptr_array(dsts), int(n_elts), int(datatype),
           int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, len(pre), _u64_array(pre),
           1 if post_op else 0, ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopyHost" if host else "nexrReduceCopy")


def make_work(srcs: Sequence[int], dsts: Sequence[int], n_elts: int, red_op_arg: int = 0,
              pre_op_args: Optional[Sequence[int]] = None, post_op: bool = False) -> ReduceCopyWork:
    """One nexrReduceCopyWork from device addresses (raises on more than 8 srcs/dsts)."""
    pre = list(pre_op_args) if pre_op_args else []
    if len(srcs) > 8 or len(dsts) > 8 or len(pre) > 8:
        raise NexrError(Result.InvalidArgument, "at most 8 srcs, dsts and preOpArgs per work")
    w = ReduceCopyWork()
    w.nSrcs, w.nDsts, w.nElts = len(srcs), len(dsts), int(n_elts)
    for i, a in enumerate(srcs):
        w.srcs[i] = int(a)
    for i, a in enumerate(dsts):
        w.dsts[i] = int(a)
    w.redOpArg = int(red_op_arg) & 0xFFFFFFFFFFFFFFFF
    w.nPreOpSrcs = len(pre)
    for i, v in enumerate(pre):
        w.preOpArgs[i] = int(v) & 0xFFFFFFFFFFFFFFFF
    w.postOp = 1 if post_op else 0
    return w


def reduce_copy_batch(works: Sequence[ReduceCopyWork], datatype: int, dev_red_op: int, stream: int = 0) -> None:
    """``nexrReduceCopyBatch``: independent reduce-copies of one (datatype, op) in few launches."""
    arr = (ReduceCopyWork * max(1, len(works)))(*works)
    _check(lib().nexrReduceCopyBatch(arr, len(works), int(datatype), int(dev_red_op),
                                     ctypes.c_void_p(int(stream)) if stream else None), "nexrReduceCopyBatch")


def reduce_copy_multi_device(works: Sequence[ReduceCopyWork], devices: Sequence[int], datatype: int,
                             dev_red_op: int, reps: int = 1) -> float:
    """``nexrReduceCopyMultiDevice``: work i on GPU devices[i], one host thread and stream per work,
    a shared start barrier, `reps` launches each. Returns seconds from the barrier to the last
    device's completion."""
    if len(works) != len(devices):
        raise NexrError(Result.InvalidArgument, "one device per work")
    arr = (ReduceCopyWork * max(1, len(works)))(*works)
    dev = (ctypes.c_int * max(1, len(devices)))(*[int(d) for d in devices])
    secs = ctypes.c_double(0.0)
    _check(lib().nexrReduceCopyMultiDevice(arr, dev, len(works), int(datatype), int(dev_red_op), int(reps),
                                           ctypes.byref(secs)), "nexrReduceCopyMultiDevice")
    return secs.value


def reduce_copy_multi_device_sets(works_per_device: Sequence[Sequence[ReduceCopyWork]], devices: Sequence[int],
                                  datatype: int, dev_red_op: int, reps: int = 1) -> float:
    """``nexrReduceCopyMultiDeviceSets``: ``works_per_device[i]`` (the same number of works for every
    entry) are rotating sets on GPU devices[i]: launch k of its thread runs set k mod len. Returns
    seconds from the start barrier to the last device's completion."""
    if len(works_per_device) != len(devices) or not works_per_device:
        raise NexrError(Result.InvalidArgument, "one list of works per device")
    n_sets = len(works_per_device[0])
    if any(len(w) != n_sets for w in works_per_device):
        raise NexrError(Result.InvalidArgument, "the same number of sets on every device")
    flat = [w for ws in works_per_device for w in ws]
    arr = (ReduceCopyWork * max(1, len(flat)))(*flat)
    dev = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
    secs = ctypes.c_double(0.0)
    _check(lib().nexrReduceCopyMultiDeviceSets(arr, dev, len(devices), n_sets, int(datatype), int(dev_red_op),
                                               int(reps), ctypes.byref(secs)), "nexrReduceCopyMultiDeviceSets")
    return secs.value


def query_launch(srcs: Sequence[int], dsts: Sequence[int], n_elts: int, datatype: int) -> LaunchInfo:
    """nexrQueryLaunch: the grid, block, cache policy and edge/body split nexrReduceCopy would use
    (no device work)."""
    info = LaunchInfo()
    _check(lib().nexrQueryLaunch(len(srcs), _ptr_array(srcs), len(dsts), _ptr_array(dsts), int(n_elts),
                                 int(datatype), ctypes.byref(info)), "nexrQueryLaunch")
    return info


def pool_stats() -> tuple:
    """(streams created by nexrReduceCopyMultiDevice, staging rings created by nexrReduceCopyHost)."""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().nexrGetPoolStats(ctypes.byref(a), ctypes.byref(b)), "nexrGetPoolStats")
    return a.value, b.value


def host_register(addr: int, nbytes: int) -> int:
    """nexrHostRegister (ncclCommRegister's counterpart for host memory): page-lock and device-map
    [addr, addr + nbytes) and record it in libnexr's registration cache. Returns the handle."""
    h = ctypes.c_void_p()
    _check(lib().nexrHostRegister(ctypes.c_void_p(int(addr)), int(nbytes), ctypes.byref(h)), "nexrHostRegister")
    return int(h.value or 0)


def host_deregister(handle: int) -> None:
    """nexrHostDeregister: drop one reference to a registration (the last one unregisters)."""
    _check(lib().nexrHostDeregister(ctypes.c_void_p(int(handle)) if handle else None), "nexrHostDeregister")


def host_mem_alloc(nbytes: int) -> int:
    """nexrHostMemAlloc (ncclMemAlloc's counterpart): pinned, device-mapped host memory."""
    p = ctypes.c_void_p()
    _check(lib().nexrHostMemAlloc(ctypes.byref(p), int(nbytes)), "nexrHostMemAlloc")
    return int(p.value)


def host_mem_free(addr: int) -> None:
    _check(lib().nexrHostMemFree(ctypes.c_void_p(int(addr)) if addr else None), "nexrHostMemFree")


def host_path_stats(reset: bool = False) -> dict:
    """nexrGetHostPathStats: where nexrReduceCopyHost calls have spent host time (ns) since the last
    reset, with the counts of calls, zero-copy calls, cache hits and runtime pointer queries."""
    st = HostPathStats()
    _check(lib().nexrGetHostPathStats(ctypes.byref(st), 1 if reset else 0), "nexrGetHostPathStats")
    return {f: int(getattr(st, f)) for f, _ in HostPathStats._fields_}


def set_semantics(mode: int) -> None:
    """nexrSetSemantics: process-wide reduction semantics for every later call (Semantics)."""
    _check(lib().nexrSetSemantics(int(mode)), "nexrSetSemantics")


def get_semantics() -> int:
    v = ctypes.c_int(-1)
    _check(lib().nexrGetSemantics(ctypes.byref(v)), "nexrGetSemantics")
    return v.value


def host_to_dev_red_op(op: int, datatype: int, n_ranks: int = 1) -> DevRedOpFull:
    """hostToDevRedOp (reference src/enqueue.cc:2185-2278) for the built-in ops."""
    out = DevRedOpFull()
    _check(lib().nexrHostToDevRedOp(ctypes.byref(out), int(op), int(datatype), int(n_ranks)), "nexrHostToDevRedOp")
    return out


def launch_one_rank(dst: int, src: int, n_elts: int, red_op: DevRedOpFull, datatype: int, stream: int = 0) -> None:
    """ncclLaunchOneRank (reference src/device/onerank.cc:48-83)."""
    _check(lib().nexrLaunchOneRank(ctypes.c_void_p(int(dst)) if dst else None,
                                   ctypes.c_void_p(int(src)) if src else None, int(n_elts), red_op,
                                   int(datatype), ctypes.c_void_p(int(stream)) if stream else None),
           "nexrLaunchOneRank")


def reduce_copy_ll(src: int, recv_lines: Sequence[int], recv_flags: Sequence[int], dst: int,
                   send_lines: Sequence[int], send_flags: Sequence[int], n_elts: int, datatype: int,
                   dev_red_op: int, red_op_arg: int = 0, src_is_input: bool = True, post_op: bool = False,
                   status: int = 0, timeout_us: int = 0, stream: int = 0) -> None:
    """One LL-protocol step (LLGenericOp, reference src/device/prims_ll.h:218-283) on device pointers."""
    u32 = ctypes.c_uint32
    rf = (u32 * max(1, len(recv_flags)))(*[int(f) & 0xFFFFFFFF for f in recv_flags])
    sf = (u32 * max(1, len(send_flags)))(*[int(f) & 0xFFFFFFFF for f in send_flags])
    rc = lib().nexrReduceCopyLL(ctypes.c_void_p(int(src)) if src else None, 1 if src_is_input else 0,
                                len(recv_lines), _ptr_array(recv_lines), rf,
                                ctypes.c_void_p(int(dst)) if dst else None, len(send_lines), _ptr_array(send_lines),
                                sf, int(n_elts), int(datatype), int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                1 if post_op else 0, ctypes.c_void_p(int(status)) if status else None,
                                int(timeout_us), ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopyLL")


def reduce_copy_ll128(src: int, recv_wire: Sequence[int], recv_flags: Sequence[int], dst: int,
                      send_wire: Sequence[int], send_flags: Sequence[int], n_elts: int, datatype: int,
                      dev_red_op: int, red_op_arg: int = 0, src_is_input: bool = True, post_op: bool = False,
                      status: int = 0, timeout_us: int = 0, stream: int = 0) -> None:
    """One LL128-protocol step (prims_ll128.h:184-331) on device pointers."""
    rf = _u64_array(list(recv_flags)) if recv_flags else None
    sf = _u64_array(list(send_flags)) if send_flags else None
    rc = lib().nexrReduceCopyLL128(ctypes.c_void_p(int(src)) if src else None, 1 if src_is_input else 0,
                                   len(recv_wire), _ptr_array(recv_wire), rf,
                                   ctypes.c_void_p(int(dst)) if dst else None, len(send_wire), _ptr_array(send_wire),
                                   sf, int(n_elts), int(datatype), int(dev_red_op),
                                   int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if post_op else 0,
                                   ctypes.c_void_p(int(status)) if status else None, int(timeout_us),
                                   ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopyLL128")


def ll_step(src_buf: int = -1, src_ix: int = 0, dst_buf: int = -1, dst_ix: int = 0, n_elts: int = 0,
            recv: bool = False, send: bool = False, post_op: bool = False, direct: int = 0) -> LLStep:
    """One step of a run (buffers: 0 input, 1 output, -1 none). direct: SIMPLE_DIRECT_RECV | SIMPLE_DIRECT_SEND,
    the ends a SIMPLE record permits to be direct (pad[0]; read by reduce_copy_simple_steps_group_direct only)."""
    s = LLStep()
    s.pad[0] = int(direct)
    s.srcIx, s.dstIx, s.nElts = int(src_ix), int(dst_ix), int(n_elts)
    s.recv, s.send, s.srcBuf, s.dstBuf, s.postOp = int(bool(recv)), int(bool(send)), int(src_buf), int(dst_buf), \
        int(bool(post_op))
    return s


def ll_conn_set(input_ptr: int, output_ptr: int, recv: Sequence[tuple], send: Sequence[tuple], slot_bytes: int,
                n_slots: int = 8) -> LLConnSet:
    """An LLConnSet from (fifo pointer, head-words pointer, step counter) per connection."""
    cs = LLConnSet()
    cs.input, cs.output = int(input_ptr) or None, int(output_ptr) or None
    cs.nRecv, cs.nSend = len(recv), len(send)
    for i, (fifo, head, step) in enumerate(recv):
        cs.recvFifo[i], cs.recvHead[i], cs.recvStep[i] = int(fifo), int(head), int(step)
    for i, (fifo, head, step) in enumerate(send):
        cs.sendFifo[i], cs.sendHead[i], cs.sendStep[i] = int(fifo), int(head), int(step)
    cs.slotBytes, cs.nSlots = int(slot_bytes), int(n_slots)
    return cs


def ll_group_workspace_bytes(n_members: int, n_launches: int = LL_GROUP_LAUNCHES) -> int:
    """Bytes of workspace for `n_launches` launches of a group of `n_members` (nexrLLGroupWorkspaceBytes
    sizes for LL_GROUP_LAUNCHES; a region per launch is that / LL_GROUP_LAUNCHES)."""
    b = ctypes.c_size_t(0)
    _check(lib().nexrLLGroupWorkspaceBytes(int(n_members), ctypes.byref(b)), "nexrLLGroupWorkspaceBytes")
    return b.value // LL_GROUP_LAUNCHES * max(1, int(n_launches))


def reduce_copy_ll_steps_group(members: Sequence[tuple], slot_bytes: int, datatype: int, dev_red_op: int,
                               red_op_arg: int = 0, n_slots: int = 8, status: int = 0, timeout_us: int = 0,
                               stream: int = 0, rule=None, workspace=None):
    """The runs of several Primitives in the same launches on one stream (nexrReduceCopyLLStepsGroup).
    members: (input_ptr, output_ptr, recv, send, steps) per member, recv / send / steps as in
    reduce_copy_ll_steps. workspace: (device pointer, bytes), or None to allocate one (a torch uint8
    tensor sized for as many launches as the longest step list has steps, the most a call can need).
    Returns the workspace tensor it allocated (None when one was given): keep it alive until the stream
    has passed the call."""
    n = len(members)
    cs = (LLConnSet * max(1, n))(*[ll_conn_set(m[0], m[1], m[2], m[3], slot_bytes, n_slots) for m in members])
    arrs = [(LLStep * max(1, len(m[4])))(*m[4]) for m in members]
    ptrs = (ctypes.POINTER(LLStep) * max(1, n))(*[ctypes.cast(a, ctypes.POINTER(LLStep)) for a in arrs])
    counts = (ctypes.c_int * max(1, n))(*[len(m[4]) for m in members])
    keep = None
    if workspace is None and 1 <= n <= LL_GROUP_MAX_MEMBERS:
        import torch
        longest = max([len(m[4]) for m in members] + [1])
        keep = torch.empty(ll_group_workspace_bytes(n, longest), dtype=torch.uint8, device="cuda")
        workspace = (keep.data_ptr(), keep.numel())
    ws_ptr, ws_bytes = workspace if workspace is not None else (0, 0)
    rc = lib().nexrReduceCopyLLStepsGroup(n, cs, ptrs, counts, int(datatype), int(dev_red_op),
                                          int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                          ctypes.byref(_ll_rule(rule)) if rule is not None else None,
                                          ctypes.c_void_p(int(status)) if status else None, int(timeout_us),
                                          ctypes.c_void_p(int(ws_ptr)) if ws_ptr else None, int(ws_bytes),
                                          ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopyLLStepsGroup")
    return keep


def reduce_copy_ll128_steps_group(members: Sequence[tuple], slot_bytes: int, datatype: int, dev_red_op: int,
                                  red_op_arg: int = 0, n_slots: int = 8, status: int = 0, timeout_us: int = 0,
                                  stream: int = 0, workspace=None):
    """LL128 step lists of several Primitives in the same launches on one stream, with the ordered
    hand-off (nexrReduceCopyLL128StepsGroup). The calling shape of reduce_copy_ll_steps_group, without a
    flag rule: slot_bytes is a multiple of 2048 and a step fills at most slot_bytes / 2048 * 1920 bytes."""
    n = len(members)
    cs = (LLConnSet * max(1, n))(*[ll_conn_set(m[0], m[1], m[2], m[3], slot_bytes, n_slots) for m in members])
    arrs = [(LLStep * max(1, len(m[4])))(*m[4]) for m in members]
    ptrs = (ctypes.POINTER(LLStep) * max(1, n))(*[ctypes.cast(a, ctypes.POINTER(LLStep)) for a in arrs])
    counts = (ctypes.c_int * max(1, n))(*[len(m[4]) for m in members])
    keep = None
    if workspace is None and 1 <= n <= LL_GROUP_MAX_MEMBERS:
        import torch
        longest = max([len(m[4]) for m in members] + [1])
        keep = torch.empty(ll_group_workspace_bytes(n, longest), dtype=torch.uint8, device="cuda")
        workspace = (keep.data_ptr(), keep.numel())
    ws_ptr, ws_bytes = workspace if workspace is not None else (0, 0)
    rc = lib().nexrReduceCopyLL128StepsGroup(n, cs, ptrs, counts, int(datatype), int(dev_red_op),
                                             int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                             ctypes.c_void_p(int(status)) if status else None, int(timeout_us),
                                             ctypes.c_void_p(int(ws_ptr)) if ws_ptr else None, int(ws_bytes),
                                             ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopyLL128StepsGroup")
    return keep


def simple_conn_set(input_ptr: int, output_ptr: int, recv: Sequence[tuple], send: Sequence[tuple], slot_bytes: int,
                    n_slots: int = 8, step_per_slice: int = 1) -> SimpleConnSet:
    """A SimpleConnSet from (fifo pointer, tail-block pointer, head-block pointer, step counter) per
    connection."""
    cs = SimpleConnSet()
    cs.input, cs.output = int(input_ptr) or None, int(output_ptr) or None
    cs.nRecv, cs.nSend = len(recv), len(send)
    for i, (fifo, tail, head, step) in enumerate(recv):
        cs.recvFifo[i], cs.recvTail[i], cs.recvHead[i], cs.recvStep[i] = int(fifo), int(tail), int(head), int(step)
    for i, (fifo, tail, head, step) in enumerate(send):
        cs.sendFifo[i], cs.sendTail[i], cs.sendHead[i], cs.sendStep[i] = int(fifo), int(tail), int(head), int(step)
    cs.slotBytes, cs.nSlots, cs.stepPerSlice = int(slot_bytes), int(n_slots), int(step_per_slice)
    return cs


def simple_group_workspace_bytes(n_members: int, n_launches: int = LL_GROUP_LAUNCHES) -> int:
    """Bytes of workspace for `n_launches` launches of a SIMPLE group of `n_members`
    (nexrSimpleGroupWorkspaceBytes sizes for LL_GROUP_LAUNCHES; a region per launch is that / LL_GROUP_LAUNCHES)."""
    b = ctypes.c_size_t(0)
    _check(lib().nexrSimpleGroupWorkspaceBytes(int(n_members), ctypes.byref(b)), "nexrSimpleGroupWorkspaceBytes")
    return b.value // LL_GROUP_LAUNCHES * max(1, int(n_launches))


def reduce_copy_simple_steps_group(members: Sequence[tuple], slot_bytes: int, datatype: int, dev_red_op: int,
                                   red_op_arg: int = 0, n_slots: int = 8, step_per_slice: int = 1,
                                   workgroups_per_member: int = 0, status: int = 0, timeout_us: int = 0,
                                   stream: int = 0, workspace=None):
    """SIMPLE step lists of several Primitives in the same launches on one stream, tails and heads in device
    memory (nexrReduceCopySimpleStepsGroup). members: (input_ptr, output_ptr, recv, send, steps) per member,
    recv / send as in simple_conn_set, steps a list of LLStep (one slice each). workspace: (device pointer,
    bytes), or None to allocate one (a torch uint8 tensor sized for one launch per step of the longest list,
    the most a call can need). Returns the workspace tensor it allocated (None when one was given): keep it
    alive until the stream has passed the call."""
    n = len(members)
    cs = (SimpleConnSet * max(1, n))(*[simple_conn_set(m[0], m[1], m[2], m[3], slot_bytes, n_slots, step_per_slice)
                                       for m in members])
    arrs = [(LLStep * max(1, len(m[4])))(*m[4]) for m in members]
    ptrs = (ctypes.POINTER(LLStep) * max(1, n))(*[ctypes.cast(a, ctypes.POINTER(LLStep)) for a in arrs])
    counts = (ctypes.c_int * max(1, n))(*[len(m[4]) for m in members])
    keep = None
    if workspace is None and 1 <= n <= LL_GROUP_MAX_MEMBERS:
        import torch
        longest = max([len(m[4]) for m in members] + [1])
        keep = torch.empty(simple_group_workspace_bytes(n, longest), dtype=torch.uint8, device="cuda")
        workspace = (keep.data_ptr(), keep.numel())
    ws_ptr, ws_bytes = workspace if workspace is not None else (0, 0)
    rc = lib().nexrReduceCopySimpleStepsGroup(n, cs, ptrs, counts, int(datatype), int(dev_red_op),
                                              int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, int(workgroups_per_member),
                                              ctypes.c_void_p(int(status)) if status else None, int(timeout_us),
                                              ctypes.c_void_p(int(ws_ptr)) if ws_ptr else None, int(ws_bytes),
                                              ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopySimpleStepsGroup")
    return keep


def simple_direct_set(send_direct: Sequence[int] = (), recv_direct: Sequence[int] = ()) -> SimpleDirectSet:
    """A SimpleDirectSet: per send connection the receiving member's output pointer (0: FIFO), per receive
    connection whether its sender writes into this member's output."""
    d = SimpleDirectSet()
    for j, ptr in enumerate(send_direct):
        d.sendDirect[j] = int(ptr) or None
    for i, on in enumerate(recv_direct):
        d.recvDirect[i] = 1 if on else 0
    return d


def simple_group_direct_workspace_bytes(n_members: int, n_launches: int = LL_GROUP_LAUNCHES) -> int:
    """simple_group_workspace_bytes for reduce_copy_simple_steps_group_direct with direct sets (its table
    entries are larger; nexrSimpleGroupDirectWorkspaceBytes)."""
    b = ctypes.c_size_t(0)
    _check(lib().nexrSimpleGroupDirectWorkspaceBytes(int(n_members), ctypes.byref(b)),
           "nexrSimpleGroupDirectWorkspaceBytes")
    return b.value // LL_GROUP_LAUNCHES * max(1, int(n_launches))


def reduce_copy_simple_steps_group_direct(members: Sequence[tuple], direct, slot_bytes: int, datatype: int,
                                          dev_red_op: int, red_op_arg: int = 0, n_slots: int = 8,
                                          step_per_slice: int = 1, workgroups_per_member: int = 0, status: int = 0,
                                          timeout_us: int = 0, stream: int = 0, workspace=None):
    """reduce_copy_simple_steps_group with DirectWrite connections (nexrReduceCopySimpleStepsGroupDirect).
    direct: None (the call is then the FIFO one), or per member a SimpleDirectSet or a (send_direct,
    recv_direct) pair as simple_direct_set takes them. The records' direct bits come from ll_step(direct=...)."""
    n = len(members)
    cs = (SimpleConnSet * max(1, n))(*[simple_conn_set(m[0], m[1], m[2], m[3], slot_bytes, n_slots, step_per_slice)
                                       for m in members])
    arrs = [(LLStep * max(1, len(m[4])))(*m[4]) for m in members]
    ptrs = (ctypes.POINTER(LLStep) * max(1, n))(*[ctypes.cast(a, ctypes.POINTER(LLStep)) for a in arrs])
    counts = (ctypes.c_int * max(1, n))(*[len(m[4]) for m in members])
    ds = None
    if direct is not None:
        ds = (SimpleDirectSet * max(1, n))(*[d if isinstance(d, SimpleDirectSet) else simple_direct_set(*d)
                                             for d in direct])
    keep = None
    if workspace is None and 1 <= n <= LL_GROUP_MAX_MEMBERS and any(len(m[4]) for m in members):
        import torch
        longest = max([len(m[4]) for m in members] + [1])
        size = simple_group_direct_workspace_bytes if direct is not None else simple_group_workspace_bytes
        keep = torch.empty(size(n, longest), dtype=torch.uint8, device="cuda")
        workspace = (keep.data_ptr(), keep.numel())
    ws_ptr, ws_bytes = workspace if workspace is not None else (0, 0)
    rc = lib().nexrReduceCopySimpleStepsGroupDirect(n, cs, ptrs, counts, int(datatype), int(dev_red_op),
                                                    int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, int(workgroups_per_member),
                                                    ds, ctypes.c_void_p(int(status)) if status else None,
                                                    int(timeout_us), ctypes.c_void_p(int(ws_ptr)) if ws_ptr else None,
                                                    int(ws_bytes), ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrReduceCopySimpleStepsGroupDirect")
    return keep


def reduce_copy_ll_steps(input_ptr: int, output_ptr: int, recv: Sequence[tuple], send: Sequence[tuple],
                         slot_bytes: int, steps: Sequence[LLStep], datatype: int, dev_red_op: int,
                         red_op_arg: int = 0, n_slots: int = 8, status: int = 0, timeout_us: int = 0,
                         stream: int = 0, rule=None) -> None:
    """A run of LL steps with device credits (nexrReduceCopyLLSteps, reference prims_ll.h:55-83 and
    :249-318). recv / send: (fifo pointer, head-words pointer, step counter) per connection. rule: an
    LLFlagRule or (flag_max, clean_mask) routes to nexrReduceCopyLLStepsRule; None is the plain call
    (the production rule)."""
    cs = LLConnSet()
    cs.input, cs.output = int(input_ptr) or None, int(output_ptr) or None
    cs.nRecv, cs.nSend = len(recv), len(send)
    for i, (fifo, head, step) in enumerate(recv):
        cs.recvFifo[i], cs.recvHead[i], cs.recvStep[i] = int(fifo), int(head), int(step)
    for i, (fifo, head, step) in enumerate(send):
        cs.sendFifo[i], cs.sendHead[i], cs.sendStep[i] = int(fifo), int(head), int(step)
    cs.slotBytes, cs.nSlots = int(slot_bytes), int(n_slots)
    arr = (LLStep * max(1, len(steps)))(*steps)
    tail = (ctypes.c_void_p(int(status)) if status else None, int(timeout_us),
            ctypes.c_void_p(int(stream)) if stream else None)
    if rule is None:
        rc = lib().nexrReduceCopyLLSteps(ctypes.byref(cs), arr, len(steps), int(datatype), int(dev_red_op),
                                         int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, *tail)
        _check(rc, "nexrReduceCopyLLSteps")
    else:
        rc = lib().nexrReduceCopyLLStepsRule(ctypes.byref(cs), arr, len(steps), int(datatype), int(dev_red_op),
                                             int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(_ll_rule(rule)),
                                             *tail)
        _check(rc, "nexrReduceCopyLLStepsRule")


SYM_MAX_RANKS = 64  # NEXR_SYM_MAX_RANKS


def sym_all_reduce(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int, n_blocks: int = 0,
                   dev_red_op: int = DevRedOp.Sum, red_op_arg: int = 0, stream: int = 0) -> None:
    """The symmetric all-reduce RSxLD_AGxST of len(inputs) ranks on one GPU in one launch (``nexrSymAllReduce``):
    rank r's device addresses inputs[r] / outputs[r], ``n_elts`` elements each of float32, float16 or bfloat16,
    Sum only. Each element is folded by its owner, its own input first, in fp32, and stored to every output;
    ``n_blocks`` (0 = 1, at most 64) is the reference's CTA count, which only decides where the passes end
    (include/nexr.h). In place allowed. Stream-ordered."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrSymAllReduce(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, int(n_blocks),
                                ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrSymAllReduce")


def sym_reduce_scatter(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                       dev_red_op: int = DevRedOp.Sum, red_op_arg: int = 0, stream: int = 0) -> None:
    """The symmetric reduce-scatter ReduceScatter_LD of len(inputs) ranks on one GPU in one launch
    (``nexrSymReduceScatter``): inputs[r] holds len(inputs) * ``n_elts`` elements of float32, float16 or
    bfloat16, outputs[r] receives chunk r folded from rank r's own input on, in fp32 with one rounding. Sum
    only. outputs[r] may be chunk r of any rank's input. Stream-ordered."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrSymReduceScatter(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                    int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                    ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrSymReduceScatter")


def sym_all_gather(inputs: Sequence[int], outputs: Sequence[int], n_bytes: int, stream: int = 0) -> None:
    """The symmetric all-gather AllGather_ST of len(inputs) ranks on one GPU in one launch
    (``nexrSymAllGather``): every outputs[s] receives the ``n_bytes`` bytes of inputs[r] at byte r * n_bytes, a
    bit copy at any alignment; a rank whose input already lies at its place in its own output skips that
    store. Stream-ordered."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrSymAllGather(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_bytes),
                                ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrSymAllGather")


FLAT_INLINE_PARTS = 120  # NEXR_FLAT_INLINE_PARTS


def flat_all_reduce(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int, dev_red_op: int,
                    red_op_arg: int, user_first: bool, parts: Sequence[tuple], stream: int = 0) -> None:
    """The ring all-reduce of len(inputs) ranks on one GPU in ONE launch with the ring's bytes
    (``nexrFlatAllReduce``): every element runs the ring's chain, one reduce-copy step per rank from its start
    rank on, in registers. ``parts`` are the channels' (offset, count, chunkCount) in elements, tiling
    [0, n_elts) in ascending order; ``user_first`` is the SIMPLE operand order (the rank's input first), False
    the LL / LL128 one. Every datatype but fp8 and every device op. In place allowed. Stream-ordered."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    arr = (FlatPart * max(1, len(parts)))(*[FlatPart(int(o), int(c), int(k)) for o, c, k in parts])
    rc = lib().nexrFlatAllReduce(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                 int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if user_first else 0, arr,
                                 len(parts), ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatAllReduce")


def flat_reduce_scatter(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int, dev_red_op: int,
                        red_op_arg: int, user_first: bool, stream: int = 0) -> None:
    """The ring reduce-scatter in ONE launch with the ring's bytes (``nexrFlatReduceScatter``): inputs[r] holds
    len(inputs) * ``n_elts`` elements, outputs[d] receives chunk d, whose chain starts at rank d + 1 and ends at
    rank d. outputs[r] may be chunk r of any input. Stream-ordered."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrFlatReduceScatter(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                     int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if user_first else 0,
                                     ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatReduceScatter")


def flat_reduce(inputs: Sequence[int], output: int, root: int, n_elts: int, datatype: int, dev_red_op: int,
                red_op_arg: int, user_first: bool, stream: int = 0) -> None:
    """The ring reduce in ONE launch with the ring's bytes (``nexrFlatReduce``): the chain starts at rank
    ``root`` + 1 and ends at ``root``, whose ``output`` alone is written. Stream-ordered."""
    rc = lib().nexrFlatReduce(len(inputs), _ptr_array(inputs), ctypes.c_void_p(int(output)) if output else None,
                              int(root), int(n_elts), int(datatype), int(dev_red_op),
                              int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if user_first else 0,
                              ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatReduce")


FLAT_GROUP_ALL_REDUCE, FLAT_GROUP_REDUCE_SCATTER, FLAT_GROUP_REDUCE, FLAT_GROUP_COPY = 0, 1, 2, 3  # NEXR_FLAT_GROUP_*
FLAT_GROUP_INLINE_BYTES = 3936  # NEXR_FLAT_GROUP_INLINE_BYTES
FLAT_GROUP_FILL_BYTES = 3968    # NEXR_FLAT_GROUP_FILL_BYTES


def flat_group_works(works: Sequence[dict]):
    """(array of nexrFlatGroupWork, keep-alive) for works given as dicts: ``coll`` (FLAT_GROUP_*), ``inputs`` and
    ``outputs`` (device addresses; a copy: one input and its destinations), ``n_elts`` (a copy: bytes), and for
    the reducing ones ``datatype``, ``dev_red_op``, ``red_op_arg`` (0), ``root`` (0) and, all-reduce only,
    ``parts`` as (offset, count, chunkCount)."""
    arr = (FlatGroupWork * max(1, len(works)))()
    keep = []
    for i, w in enumerate(works):
        ins, outs = _ptr_array(w["inputs"]), _ptr_array(w["outputs"])
        parts = w.get("parts") or ()
        pa = (FlatPart * max(1, len(parts)))(*[FlatPart(int(o), int(c), int(k)) for o, c, k in parts])
        keep += [ins, outs, pa]
        arr[i] = FlatGroupWork(int(w["coll"]), int(w.get("datatype", 0)), int(w.get("dev_red_op", 0)),
                               int(w.get("root", 0)), int(w.get("red_op_arg", 0)) & 0xFFFFFFFFFFFFFFFF,
                               ctypes.cast(ins, ctypes.POINTER(ctypes.c_void_p)),
                               ctypes.cast(outs, ctypes.POINTER(ctypes.c_void_p)), len(w["outputs"]), len(parts), pa,
                               int(w["n_elts"]))
    return arr, keep


def _flat_group(plan_only: bool, n_ranks: int, works: Sequence[dict], user_first: bool, max_workgroups: int,
                stream: int):
    arr, keep = flat_group_works(works)
    launch_of = (ctypes.c_int * max(1, len(works)))()
    info = FlatGroupInfo()
    args = [int(n_ranks), arr, len(works), 1 if user_first else 0, int(max_workgroups), launch_of, ctypes.byref(info)]
    if plan_only:
        _check(lib().nexrFlatGroupPlan(*args), "nexrFlatGroupPlan")
    else:
        _check(lib().nexrFlatGroup(*args, ctypes.c_void_p(int(stream)) if stream else None), "nexrFlatGroup")
    del keep
    return list(launch_of[:len(works)]), {"works": info.works, "launches": info.launches,
                                          "fill_launches": info.fillLaunches, "cuts": info.cuts, "table_bytes": info.tableBytes,
                                          "workgroups": info.workgroups}


def flat_group(n_ranks: int, works: Sequence[dict], user_first: bool, max_workgroups: int = 0, stream: int = 0):
    """Several flat collectives as flat GROUP launches (``nexrFlatGroup``): the bytes of the same works issued in
    order through flat_all_reduce / flat_reduce_scatter / flat_reduce / flat_broadcast, one launch per (datatype,
    op, min-or-max) and one for copies between two conflicts. ``works`` as flat_group_works takes them. Returns
    (launch_of, info): the launch of every work (-1: empty) and the counts. Stream-ordered."""
    return _flat_group(False, n_ranks, works, user_first, max_workgroups, stream)


def flat_group_plan(n_ranks: int, works: Sequence[dict], user_first: bool, max_workgroups: int = 0):
    """flat_group's validation and launch plan without any device call (``nexrFlatGroupPlan``)."""
    return _flat_group(True, n_ranks, works, user_first, max_workgroups, 0)


FLAT_TREE_SLOTS = 8          # NEXR_FLAT_TREE_SLOTS
FLAT_TREE_INLINE_PARTS = 96  # NEXR_FLAT_TREE_INLINE_PARTS


def flat_tree_links(trees: Sequence[Sequence[tuple]]):
    """(array of nexrFlatTreeLinks pointers, keep-alive) for ``trees[t][r] = (up, [down...])``."""
    rows = []
    for links in trees:
        row = (FlatTreeLinks * max(1, len(links)))()
        for r, (up, down) in enumerate(links):
            d = [int(x) for x in down] + [-1] * (3 - len(down))
            row[r] = FlatTreeLinks(int(up), (ctypes.c_int * 3)(*d[:3]))
        rows.append(row)
    arr = (ctypes.POINTER(FlatTreeLinks) * max(1, len(rows)))(
        *[ctypes.cast(row, ctypes.POINTER(FlatTreeLinks)) for row in rows])
    return arr, rows


def flat_tree_all_reduce(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int, dev_red_op: int,
                         red_op_arg: int, user_first: bool, trees: Sequence[Sequence[tuple]], parts: Sequence[tuple],
                         stream: int = 0) -> None:
    """The tree all-reduce of len(inputs) ranks on one GPU in ONE launch with the FIFO tree's bytes
    (``nexrFlatTreeAllReduce``): every rank's one reduce-copy step over its own input and its children's values
    in down[] order, interpreted in registers. ``trees[t][r] = (up, [down...])`` (one or two trees), ``parts``
    are the channels' (offset, count, tree) in elements, tiling [0, n_elts) in ascending order; ``user_first``
    is the SIMPLE operand order, False the LL / LL128 one. In place allowed. Stream-ordered."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    tarr, _keep = flat_tree_links(trees)
    arr = (FlatTreePart * max(1, len(parts)))(*[FlatTreePart(int(o), int(c), int(t), 0) for o, c, t in parts])
    rc = lib().nexrFlatTreeAllReduce(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                     int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if user_first else 0,
                                     tarr, len(trees), arr, len(parts),
                                     ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatTreeAllReduce")


FLAT_PREMUL_INLINE_PARTS = 96       # NEXR_FLAT_PREMUL_INLINE_PARTS
FLAT_TREE_PREMUL_INLINE_PARTS = 64  # NEXR_FLAT_TREE_PREMUL_INLINE_PARTS


def _scalar_array(scalars: Optional[Sequence[int]]):
    if scalars is None:
        return None
    return (ctypes.c_uint64 * max(1, len(scalars)))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in scalars])


def flat_all_reduce_premul(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                           scalars: Optional[Sequence[int]], scalars_are_ptrs: bool, user_first: bool,
                           parts: Sequence[tuple], stream: int = 0) -> None:
    """``flat_all_reduce`` under PreMulSum with a scalar per rank (``nexrFlatAllReducePreMul``): rank r's input is
    multiplied by ``scalars[r]``, the raw bits of one element, or with ``scalars_are_ptrs`` the device address
    the kernel reads it from (no host read: a copy queued on the stream before the launch is seen)."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    arr = (FlatPart * max(1, len(parts)))(*[FlatPart(int(o), int(c), int(k)) for o, c, k in parts])
    rc = lib().nexrFlatAllReducePreMul(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts),
                                       int(datatype), _scalar_array(scalars), 1 if scalars_are_ptrs else 0,
                                       1 if user_first else 0, arr, len(parts),
                                       ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatAllReducePreMul")


def flat_reduce_scatter_premul(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                               scalars: Optional[Sequence[int]], scalars_are_ptrs: bool, user_first: bool,
                               stream: int = 0) -> None:
    """``flat_reduce_scatter`` with a scalar per rank (``nexrFlatReduceScatterPreMul``), as flat_all_reduce_premul."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrFlatReduceScatterPreMul(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts),
                                           int(datatype), _scalar_array(scalars), 1 if scalars_are_ptrs else 0,
                                           1 if user_first else 0, ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatReduceScatterPreMul")


def flat_reduce_premul(inputs: Sequence[int], output: int, root: int, n_elts: int, datatype: int,
                       scalars: Optional[Sequence[int]], scalars_are_ptrs: bool, user_first: bool,
                       stream: int = 0) -> None:
    """``flat_reduce`` with a scalar per rank (``nexrFlatReducePreMul``), as flat_all_reduce_premul."""
    rc = lib().nexrFlatReducePreMul(len(inputs), _ptr_array(inputs), ctypes.c_void_p(int(output)) if output else None,
                                    int(root), int(n_elts), int(datatype), _scalar_array(scalars),
                                    1 if scalars_are_ptrs else 0, 1 if user_first else 0,
                                    ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatReducePreMul")


def flat_tree_all_reduce_premul(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                                scalars: Optional[Sequence[int]], scalars_are_ptrs: bool, user_first: bool,
                                trees: Sequence[Sequence[tuple]], parts: Sequence[tuple], stream: int = 0) -> None:
    """``flat_tree_all_reduce`` with a scalar per rank (``nexrFlatTreeAllReducePreMul``), as
    flat_all_reduce_premul."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    tarr, _keep = flat_tree_links(trees)
    arr = (FlatTreePart * max(1, len(parts)))(*[FlatTreePart(int(o), int(c), int(t), 0) for o, c, t in parts])
    rc = lib().nexrFlatTreeAllReducePreMul(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts),
                                           int(datatype), _scalar_array(scalars), 1 if scalars_are_ptrs else 0,
                                           1 if user_first else 0, tarr, len(trees), arr, len(parts),
                                           ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatTreeAllReducePreMul")


def flat_broadcast(input: int, outputs: Sequence[int], n_bytes: int, stream: int = 0) -> None:
    """The broadcast in ONE launch (``nexrFlatBroadcast``): ``n_bytes`` of ``input`` to every output whose address
    differs from it, a bit copy at any byte alignment. Stream-ordered."""
    rc = lib().nexrFlatBroadcast(len(outputs), ctypes.c_void_p(int(input)) if input else None, _ptr_array(outputs),
                                 int(n_bytes), ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrFlatBroadcast")


# ---- the flat collectives over host memory (nexrFlatHost*): the device forms' arguments, host addresses -------------
def _stream_arg(stream: int):
    return ctypes.c_void_p(int(stream)) if stream else None


def flat_host_all_reduce(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int, dev_red_op: int,
                         red_op_arg: int, user_first: bool, parts: Sequence[tuple], stream: int = 0) -> None:
    """``flat_all_reduce`` over HOST buffers (``nexrFlatHostAllReduce``): pinned buffers are read and written in
    place over the link in one launch, pageable ones are staged (a window pipeline beyond
    NEXR_FLAT_HOST_CHUNK_BYTES). Returns when the outputs are complete."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    arr = (FlatPart * max(1, len(parts)))(*[FlatPart(int(o), int(c), int(k)) for o, c, k in parts])
    rc = lib().nexrFlatHostAllReduce(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                     int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if user_first else 0,
                                     arr, len(parts), _stream_arg(stream))
    _check(rc, "nexrFlatHostAllReduce")


def flat_host_reduce_scatter(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                             dev_red_op: int, red_op_arg: int, user_first: bool, stream: int = 0) -> None:
    """``flat_reduce_scatter`` over HOST buffers (``nexrFlatHostReduceScatter``); pageable buffers are staged
    whole. Returns when the outputs are complete."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrFlatHostReduceScatter(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts),
                                         int(datatype), int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                         1 if user_first else 0, _stream_arg(stream))
    _check(rc, "nexrFlatHostReduceScatter")


def flat_host_reduce(inputs: Sequence[int], output: int, root: int, n_elts: int, datatype: int, dev_red_op: int,
                     red_op_arg: int, user_first: bool, stream: int = 0) -> None:
    """``flat_reduce`` over HOST buffers (``nexrFlatHostReduce``). Returns when the output is complete."""
    rc = lib().nexrFlatHostReduce(len(inputs), _ptr_array(inputs), ctypes.c_void_p(int(output)) if output else None,
                                  int(root), int(n_elts), int(datatype), int(dev_red_op),
                                  int(red_op_arg) & 0xFFFFFFFFFFFFFFFF, 1 if user_first else 0, _stream_arg(stream))
    _check(rc, "nexrFlatHostReduce")


def flat_host_tree_all_reduce(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                              dev_red_op: int, red_op_arg: int, user_first: bool, trees: Sequence[Sequence[tuple]],
                              parts: Sequence[tuple], stream: int = 0) -> None:
    """``flat_tree_all_reduce`` over HOST buffers (``nexrFlatHostTreeAllReduce``). Returns when the outputs are
    complete."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    tarr, _keep = flat_tree_links(trees)
    arr = (FlatTreePart * max(1, len(parts)))(*[FlatTreePart(int(o), int(c), int(t), 0) for o, c, t in parts])
    rc = lib().nexrFlatHostTreeAllReduce(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts),
                                         int(datatype), int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                         1 if user_first else 0, tarr, len(trees), arr, len(parts), _stream_arg(stream))
    _check(rc, "nexrFlatHostTreeAllReduce")


def flat_host_broadcast(input: int, outputs: Sequence[int], n_bytes: int, stream: int = 0) -> None:
    """``flat_broadcast`` over HOST buffers (``nexrFlatHostBroadcast``). Returns when the outputs are complete."""
    rc = lib().nexrFlatHostBroadcast(len(outputs), ctypes.c_void_p(int(input)) if input else None,
                                     _ptr_array(outputs), int(n_bytes), _stream_arg(stream))
    _check(rc, "nexrFlatHostBroadcast")


def flat_host_all_gather(inputs: Sequence[int], outputs: Sequence[int], n_bytes: int, stream: int = 0) -> None:
    """``sym_all_gather``'s bytes over HOST buffers (``nexrFlatHostAllGather``): outputs[s][r * n_bytes + b] =
    inputs[r][b]; pageable buffers are staged whole. Returns when the outputs are complete."""
    if len(inputs) != len(outputs):
        raise NexrError(Result.InvalidArgument, "one input and one output per rank")
    rc = lib().nexrFlatHostAllGather(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_bytes),
                                     _stream_arg(stream))
    _check(rc, "nexrFlatHostAllGather")


def flat_host_stats(reset: bool = False) -> dict:
    """nexrGetFlatHostStats: how the nexrFlatHost* calls since the last reset classified and staged their buffers
    (process-wide)."""
    st = FlatHostStats()
    _check(lib().nexrGetFlatHostStats(ctypes.byref(st), 1 if reset else 0), "nexrGetFlatHostStats")
    return {f: int(getattr(st, f)) for f, _ in FlatHostStats._fields_}


SYM_LL_HEADER_BYTES = 256  # NEXR_SYM_LL_HEADER_BYTES
SYM_LL_ROUND_PACKS = 256   # NEXR_SYM_LL_ROUND_PACKS
SYM_LL_MAX_BLOCKS = 64     # NEXR_SYM_LL_MAX_BLOCKS


def sym_ll_window_bytes(n_ranks: int, max_blocks: int) -> int:
    """Bytes of one rank's window of the symmetric LL calls for ``n_ranks`` ranks and up to ``max_blocks`` blocks
    (``nexrSymLLWindowBytes``): the header of 64 epoch words, then per block two buffers of
    n_ranks * SYM_LL_ROUND_PACKS 16-byte lines. A window is device memory, zeroed once."""
    out = ctypes.c_size_t()
    _check(lib().nexrSymLLWindowBytes(int(n_ranks), int(max_blocks), ctypes.byref(out)), "nexrSymLLWindowBytes")
    return out.value


def _sym_ll_tail(windows, window_bytes, n_blocks, status, timeout_us, stream):
    return (_ptr_array(windows), int(window_bytes), int(n_blocks), ctypes.c_void_p(int(status)) if status else None,
            int(timeout_us), ctypes.c_void_p(int(stream)) if stream else None)


def sym_ll_all_reduce(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                      windows: Sequence[int], window_bytes: int, n_blocks: int = 0, status: int = 0,
                      timeout_us: int = 0, dev_red_op: int = DevRedOp.Sum, red_op_arg: int = 0,
                      stream: int = 0) -> None:
    """The symmetric LL all-reduce AllReduce_AGxLL_R of len(inputs) ranks on one GPU in one launch
    (``nexrSymLLAllReduce``): every rank's packs travel as flagged 16-byte lines into every rank's window, and
    every output element is inputs[0] + inputs[1] + ... in rank order, in fp32 with one rounding. float32,
    float16 or bfloat16, Sum only, fewer than 2 GiB. ``windows[r]`` is rank r's zeroed window of
    ``window_bytes`` >= sym_ll_window_bytes(n, n_blocks); ``status`` / ``timeout_us`` as reduce_copy_ll. In
    place allowed. Stream-ordered."""
    if len(inputs) != len(outputs) or len(inputs) != len(windows):
        raise NexrError(Result.InvalidArgument, "one input, one output and one window per rank")
    rc = lib().nexrSymLLAllReduce(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts), int(datatype),
                                  int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                  *_sym_ll_tail(windows, window_bytes, n_blocks, status, timeout_us, stream))
    _check(rc, "nexrSymLLAllReduce")


def sym_ll_reduce_scatter(inputs: Sequence[int], outputs: Sequence[int], n_elts: int, datatype: int,
                          windows: Sequence[int], window_bytes: int, n_blocks: int = 0, status: int = 0,
                          timeout_us: int = 0, dev_red_op: int = DevRedOp.Sum, red_op_arg: int = 0,
                          stream: int = 0) -> None:
    """The symmetric LL reduce-scatter ReduceScatter_LL (``nexrSymLLReduceScatter``): inputs[r] holds
    len(inputs) * ``n_elts`` elements, outputs[r] receives chunk r folded from rank 0's input on in rank order,
    in fp32 with one rounding. outputs[r] may be chunk r of inputs[r]. Windows, status and timeout as
    sym_ll_all_reduce. Stream-ordered."""
    if len(inputs) != len(outputs) or len(inputs) != len(windows):
        raise NexrError(Result.InvalidArgument, "one input, one output and one window per rank")
    rc = lib().nexrSymLLReduceScatter(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_elts),
                                      int(datatype), int(dev_red_op), int(red_op_arg) & 0xFFFFFFFFFFFFFFFF,
                                      *_sym_ll_tail(windows, window_bytes, n_blocks, status, timeout_us, stream))
    _check(rc, "nexrSymLLReduceScatter")


def sym_ll_all_gather(inputs: Sequence[int], outputs: Sequence[int], n_bytes: int, windows: Sequence[int],
                      window_bytes: int, n_blocks: int = 0, status: int = 0, timeout_us: int = 0,
                      stream: int = 0) -> None:
    """The symmetric LL all-gather AllGather_LL (``nexrSymLLAllGather``): every outputs[s] receives the
    ``n_bytes`` bytes of inputs[r] at byte r * n_bytes, a bit copy at any alignment, through the windows'
    lines. inputs[r] may lie at its place in outputs[r]. Windows, status and timeout as sym_ll_all_reduce.
    Stream-ordered."""
    if len(inputs) != len(outputs) or len(inputs) != len(windows):
        raise NexrError(Result.InvalidArgument, "one input, one output and one window per rank")
    rc = lib().nexrSymLLAllGather(len(inputs), _ptr_array(inputs), _ptr_array(outputs), int(n_bytes),
                                  *_sym_ll_tail(windows, window_bytes, n_blocks, status, timeout_us, stream))
    _check(rc, "nexrSymLLAllGather")


def ll_clean_slot(send_lines: Sequence[int], send_flags: Sequence[int], first_line: int, slot_lines: int,
                  stream: int = 0) -> None:
    """nexrLLCleanSlot: lines [first_line, slot_lines) of each slot become {0, flag, 0, flag} — what the
    caller of the single-step reduce_copy_ll queues behind it on a cleaning step (ll_cleans)."""
    sf = (ctypes.c_uint32 * max(1, len(send_flags)))(*[int(f) & 0xFFFFFFFF for f in send_flags])
    rc = lib().nexrLLCleanSlot(len(send_lines), _ptr_array(send_lines), sf, int(first_line), int(slot_lines),
                               ctypes.c_void_p(int(stream)) if stream else None)
    _check(rc, "nexrLLCleanSlot")


def version() -> int:
    return lib().nexrGetVersion()


# ---- torch convenience layer (device memory and streams only; the compute is libnexr) ----------
def torch_datatype(dtype) -> DataType:
    import torch
    m = {torch.int8: DataType.Int8, torch.uint8: DataType.Uint8, torch.int32: DataType.Int32,
         torch.int64: DataType.Int64, torch.float16: DataType.Float16, torch.float32: DataType.Float32,
         torch.float64: DataType.Float64, torch.bfloat16: DataType.Bfloat16}
    for name, dt in (("uint32", DataType.Uint32), ("uint64", DataType.Uint64)):
        t = getattr(torch, name, None)
        if t is not None:
            m[t] = dt
    if dtype not in m:
        raise NexrError(Result.InvalidArgument, f"unsupported torch dtype {dtype}")
    return m[dtype]


def reduce_copy(srcs, dsts, dev_red_op: int = DevRedOp.Sum, red_op_arg: int = 0,
                pre_op_args: Optional[Sequence[int]] = None, post_op: bool = False, datatype: Optional[int] = None,
                stream=None) -> None:
    """Reduce-copy over torch tensors on one device: every dst[i] = fold(srcs)[i].

    All tensors must be contiguous with the same element count. ``datatype`` defaults to the
    tensors' dtype (pass ``DataType.Uint32``/``Uint64`` explicitly for unsigned views of int32/int64
    storage). ``stream`` is a torch stream (default: the current stream)."""
    import torch
    if not srcs:
        raise NexrError(Result.InvalidArgument, "no sources")
    n = srcs[0].numel()
    for t in list(srcs) + list(dsts):
        if not t.is_contiguous() or t.numel() != n:
            raise NexrError(Result.InvalidArgument, "tensors must be contiguous and equally sized")
    dt = torch_datatype(srcs[0].dtype) if datatype is None else DataType(datatype)
    if stream is None and srcs[0].is_cuda:
        stream = torch.cuda.current_stream(srcs[0].device)
    handle = stream.cuda_stream if stream is not None else 0
    reduce_copy_ptrs([t.data_ptr() for t in srcs], [t.data_ptr() for t in dsts], n, dt, dev_red_op,
                     red_op_arg, pre_op_args, post_op, handle, host=not srcs[0].is_cuda)
