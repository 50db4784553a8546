/*
 * nexr.h — C ABI of the MI355X-native reduce-copy primitive.
 *
 * This is the drop-in boundary for the one hot path of MJChku/nex-nccl this project rebuilds:
 * the element-wise K-source / M-destination reduce-copy that every collective's payload goes
 * through (reference: src/device/common_kernel.h:269-349 `reduceCopy`, inner loop
 * `reduceCopyPacks` :32-267, element arithmetic src/device/reduce_kernel.h:427-592).
 *
 * Plain C: pointers, sizes and integer enums only. Every enum value is numerically identical to
 * the reference so a caller can pass its own ncclDataType_t / ncclDevRedOp_t / ncclResult_t
 * values straight through.
 *
 * Ownership and ordering (reference src/enqueue.cc:1543-1640, src/device/onerank.cc:48-83):
 *   - the caller owns every buffer; nothing is allocated or freed inside a hot call;
 *   - device calls are stream-ordered and asynchronous on the given HIP stream (NULL = the
 *     default stream of the current device); they never synchronise the host;
 *   - calls are safe concurrently on different devices / streams (no global mutable state apart
 *     from the process-wide reduction semantics below, set before the first call: tuning knobs are
 *     read from the environment once; host staging resources are pooled per device);
 *   - errors are returned, never aborted on.
 */
#ifndef NEXR_H_
#define NEXR_H_

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define NEXR_API __attribute__((visibility("default")))

/* 0.3.0 also covers the LL flag rule (nexrLLFlagRule, nexrReduceCopyLLStepsRule, nexrLLCleanSlot) and the
 * group launches (nexrLLGroupWorkspaceBytes, nexrReduceCopyLLStepsGroup, nexrReduceCopyLL128StepsGroup
 * for LL128 step lists, and nexrSimpleGroupWorkspaceBytes / nexrReduceCopySimpleStepsGroup with
 * nexrSimpleConnSet for SIMPLE ones, nexrSimpleGroupDirectWorkspaceBytes / nexrReduceCopySimpleStepsGroupDirect
 * with nexrSimpleDirectSet for their DirectWrite form) and the symmetric all-reduce, reduce-scatter and
 * all-gather (nexrSymAllReduce, nexrSymReduceScatter, nexrSymAllGather): additions only, no existing entry point or struct layout changed, so the version
 * stays. */
#define NEXR_VERSION_MAJOR 0
#define NEXR_VERSION_MINOR 3
#define NEXR_VERSION_PATCH 0

/* Maximum fan-in / fan-out of one call: srcs[]/dsts[] hold NCCL_MAX_ARITY+1 = 8 entries
 * (reference src/device/common.h:101-102, src/include/device.h:816,:842-846). */
#define NEXR_MAX_SRCS 8
#define NEXR_MAX_DSTS 8

/* Result codes — identical to ncclResult_t (reference src/nccl.h.in:40-48). */
typedef enum {
  nexrSuccess = 0,
  nexrUnhandledCudaError = 1, /* any hipError_t from the runtime */
  nexrSystemError = 2,
  nexrInternalError = 3,
  nexrInvalidArgument = 4,    /* bad K/M/dtype/op/null pointer/unsupported combination */
  nexrInvalidUsage = 5,
  nexrRemoteError = 6,
  nexrInProgress = 7,
  nexrNumResults = 8
} nexrResult_t;

/* Data types — identical to ncclDataType_t (reference src/nccl.h.in:278-290). */
typedef enum {
  nexrInt8 = 0, nexrChar = 0,
  nexrUint8 = 1,
  nexrInt32 = 2, nexrInt = 2,
  nexrUint32 = 3,
  nexrInt64 = 4,
  nexrUint64 = 5,
  nexrFloat16 = 6, nexrHalf = 6,
  nexrFloat32 = 7, nexrFloat = 7,
  nexrFloat64 = 8, nexrDouble = 8,
  nexrBfloat16 = 9,
  nexrFloat8e4m3 = 10, /* declared for enum parity; the fork never compiles its fp8 path
                          (reduce_kernel.h:17 guard), so calls return nexrInvalidArgument */
  nexrFloat8e5m2 = 11,
  nexrNumTypes = 12
} nexrDataType_t;

/* User-level reduction ops — identical to ncclRedOp_t (reference src/nccl.h.in:259-270). */
typedef enum { nexrSum = 0, nexrProd = 1, nexrMax = 2, nexrMin = 3, nexrAvg = 4, nexrNumOps = 5 } nexrRedOp_t;

/* Device reduction ops — identical to ncclDevRedOp_t (reference src/include/device.h:683-687). */
typedef enum {
  nexrDevSum = 0,
  nexrDevProd = 1,
  nexrDevMinMax = 2,     /* redOpArg bit 0: 0 = min, 1 = max (reduce_kernel.h:64) */
  nexrDevPreMulSum = 3,  /* preOp: x * scalar (scalar = raw bits of T in preOpArgs[s]) */
  nexrDevSumPostDiv = 4, /* integer types only; redOpArg = divisor<<1 | isSigned. isSigned alone, not the
                          * datatype, selects the signed quotient (reduce_kernel.h:79-97), which divides by the
                          * divisor truncated to T: a 1-byte type with isSigned set and a divisor whose low
                          * byte is 0 is nexrInvalidArgument; with isSigned clear every divisor is valid. */
  nexrNumDevRedOps = 5
} nexrDevRedOp_t;

/* Byte-exact mirror of struct ncclDevRedOpFull (reference src/include/device.h:688-693):
 * two 4-byte enums at offsets 0 and 4, a one-byte bool at offset 8 (bytes 9-15 are padding the
 * library never reads), the 64-bit scalar at offset 16; sizeof == 24. tests/test_abi.py checks the
 * layout against a C restatement of the reference struct. */
typedef struct {
  int op;               /* nexrDevRedOp_t (ncclDevRedOp_t, an int-sized enum) */
  int proxyOp;          /* nexrRedOp_t the user asked for */
  bool scalarArgIsPtr;  /* scalarArg holds a device pointer to the scalar (onerank.cc:32-42) */
  uint64_t scalarArg;
} nexrDevRedOpFull;

typedef void* nexrStream_t; /* a hipStream_t; NULL = default stream */

/*
 * nexrReduceCopy — replaces the device primitive
 *   reduceCopy<Unroll,RedFn,T,0,MinSrcs,MaxSrcs,0,MinDsts,MaxDsts,PreOpSrcs>(
 *       thread, nThreads, redArg, preOpArgs, postOp, nSrcs, srcPtrs, nDsts, dstPtrs, nElts)
 * (reference src/device/common_kernel.h:331-349), called by genericOp at
 * src/device/prims_simple.h:264,:272,:282,:290 and by oneRankReduce at src/device/onerank.cc:43.
 *
 * For every element i in [0, nElts):
 *   acc = srcs[0][i]              (then acc = acc * preOpArgs[0]   if 0 < nPreOpSrcs, PreMulSum)
 *   for s in 1..nSrcs-1:
 *     v = srcs[s][i]              (then v   = v   * preOpArgs[s]   if s < nPreOpSrcs, PreMulSum)
 *     acc = reduce(acc, v)        (acc is the FIRST operand: reduce_kernel.h:152-168)
 *   if postOp: acc = acc / divisor                                  (SumPostDiv)
 *   dsts[d][i] = acc for every d
 * with the per-type scalar arithmetic of reduce_kernel.h:238-539 (real arithmetic, i.e. the
 * fork's SKIP_COMP at reduce_kernel.h:432 removed; Min/Max compared at the signedness of
 * `datatype`). Rounding to T after every step; integer sum/prod wrap modulo 2^bits.
 *
 * Device pointers; any alignment; dsts may alias srcs[0] exactly (in-place). nElts == 0 or
 * nDsts == 0 is a no-op (common_kernel.h:288-289). 1 <= nSrcs <= 8, 0 <= nDsts <= 8,
 * 0 <= nPreOpSrcs <= nSrcs, preOpArgs may be NULL when nPreOpSrcs == 0.
 */
NEXR_API nexrResult_t nexrReduceCopy(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                     size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                     int nPreOpSrcs, const uint64_t* preOpArgs, int postOp,
                                     nexrStream_t stream);

/*
 * nexrReduceCopyBatch — many independent reduce-copies of one (datatype, devRedOp) in as few
 * launches as possible: the analogue of a kernel launch carrying a batch of works in its 4 KiB
 * argument block (reference src/include/device.h:1074-1098 ncclDevKernelArgs4K,
 * src/device/common.h:165-200 loadWorkBatchToShmem, :424-445 the per-block work loop). Each work
 * has exactly the semantics of one nexrReduceCopy call with its own fields. Works with the same
 * nSrcs share a launch (at most NEXR_MAX_BATCH_WORKS per launch); each work gets workgroups in
 * proportion to its size. Works run concurrently in no defined order, so no work's dsts may overlap
 * another work's srcs or dsts (in-place within one work is allowed). Every work is validated
 * before anything is launched: on an argument error nothing runs. Works with nElts == 0 or
 * nDsts == 0 are skipped. Small messages are launch-bound (~4 us per nexrReduceCopy call on
 * MI355X); a batch pays that once per launch.
 */
#define NEXR_MAX_BATCH_WORKS 14
typedef struct {
  int nSrcs;
  int nDsts;
  const void* srcs[NEXR_MAX_SRCS];
  void* dsts[NEXR_MAX_DSTS];
  size_t nElts;
  uint64_t redOpArg;
  int nPreOpSrcs;
  int postOp;
  uint64_t preOpArgs[NEXR_MAX_SRCS];
} nexrReduceCopyWork;

NEXR_API nexrResult_t nexrReduceCopyBatch(const nexrReduceCopyWork* works, int nWorks, int datatype, int devRedOp,
                                          nexrStream_t stream);

/*
 * nexrReduceCopyMultiDevice — independent reduce-copies on several GPUs of one node from one host
 * call: the independent-chunk sharding of SURVEY §8(e) (config C5) as a native host driver, with no
 * collective and no peer access. Work i runs on HIP device devices[i] (its buffers live there) on a
 * host thread of its own: hipSetDevice, a non-blocking stream of its own (checked out of a
 * process-wide per-device pool and handed back drained), a start barrier shared by all works, then `reps` reduce-copies (each exactly one nexrReduceCopy of work i) and
 * hipStreamSynchronize. Every work and device ordinal is validated before any thread starts; the
 * first error of any work is returned. When `seconds` is non-null it receives the wall time from the
 * barrier's release to the last device's completion. The caller's current device is unchanged. Works
 * must not overlap one another (in-place within one work is allowed). At most
 * NEXR_MAX_MULTI_DEVICE_WORKS works; several may name the same device.
 */
#define NEXR_MAX_MULTI_DEVICE_WORKS 64
NEXR_API nexrResult_t nexrReduceCopyMultiDevice(const nexrReduceCopyWork* works, const int* devices, int nWorks,
                                                int datatype, int devRedOp, int reps, double* seconds);

/*
 * nexrReduceCopyMultiDeviceSets — nexrReduceCopyMultiDevice with nSets rotating works per thread:
 * works[i * nSets + s] (s < nSets) all run on devices[i], and launch k (k < reps) of thread i is
 * work i * nSets + k mod nSets. With nSets buffer sets per GPU, consecutive launches never re-read
 * the previous launch's cache-resident bytes (the N = 1 bench's rotation, applied to C5). nSets = 1
 * is nexrReduceCopyMultiDevice. Validation, threads, streams, barrier and timing as above.
 */
#define NEXR_MAX_MULTI_DEVICE_SETS 8
NEXR_API nexrResult_t nexrReduceCopyMultiDeviceSets(const nexrReduceCopyWork* works, const int* devices, int nWorks,
                                                    int nSets, int datatype, int devRedOp, int reps, double* seconds);

/*
 * nexrReduceCopyHost — the same reduce-copy for buffers in HOST memory (the emulated
 * transport's staging FIFOs, reference src/include/device.h:753-771): copies the K inputs
 * host->device, runs nexrReduceCopy, copies the M outputs device->host, and synchronises the
 * stream before returning. Device scratch is a staging ring checked out of a process-wide,
 * per-device pool for the duration of the call and handed back at its end (grown on demand; the
 * only call that may allocate), so callers on short-lived threads reuse the same rings. When every buffer is pinned host memory (hipHostMalloc /
 * hipHostRegister / torch pin_memory) the kernel reads and writes it in place over PCIe (zero-copy,
 * both directions concurrently; NEXR_HOST_ZERO_COPY=0 disables). Otherwise the call stages through
 * device memory in chunks (NEXR_HOST_CHUNK_BYTES, default 8 MiB per buffer): chunk c is copied in
 * and reduced while chunk c-1 is copied out on a second stream.
 */
NEXR_API nexrResult_t nexrReduceCopyHost(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                         size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                         int nPreOpSrcs, const uint64_t* preOpArgs, int postOp,
                                         nexrStream_t stream);

/*
 * Host-memory registration — replaces ncclCommRegister / ncclCommDeregister (reference
 * src/nccl.h.in:243-246, src/register/register.cc:128-170) and ncclMemAlloc / ncclMemFree
 * (src/nccl.h.in:130-133, src/allocator.cc) for the fork's setting, where NEX "device memory" and
 * the transport's staging FIFOs are host memory.
 *   nexrHostRegister    page-locks and device-maps [buff, buff + size) (hipHostRegister, mapped +
 *                       portable) and records it in a process-wide cache sorted by address, like the
 *                       reference's regCache (register.cc:40-60). A range inside an entry already here
 *                       (registered, or from nexrHostMemAlloc) shares that entry (one more reference);
 *                       a range that partly overlaps one returns nexrInvalidUsage. Disjoint ranges that
 *                       share a page are separate entries (the runtime maps each; if it refused one,
 *                       nexrInvalidUsage). *handle is an opaque id that is never reused.
 *   nexrHostDeregister  drops one reference; the last one unregisters the range (NULL: no-op). A
 *                       handle with no reference left, or never issued, returns nexrInvalidUsage.
 *   nexrHostMemAlloc    pinned, device-mapped host memory (hipHostMalloc), recorded in the same cache.
 *   nexrHostMemFree     frees memory from nexrHostMemAlloc (NULL: no-op); nexrInvalidUsage while
 *                       registrations inside it remain (deregister them first).
 * nexrReduceCopyHost looks every buffer up in this cache first: a buffer wholly inside an entry is
 * read and written in place over PCIe with no runtime query. Other pinned memory (registered by the
 * caller directly) is still found with hipPointerGetAttributes on every call. Do not free or
 * unregister a range behind the library's back while it is registered here.
 */
NEXR_API nexrResult_t nexrHostRegister(void* buff, size_t size, void** handle);
NEXR_API nexrResult_t nexrHostDeregister(void* handle);
NEXR_API nexrResult_t nexrHostMemAlloc(void** ptr, size_t size);
NEXR_API nexrResult_t nexrHostMemFree(void* ptr);

/*
 * nexrGetHostPathStats — diagnostics: where nexrReduceCopyHost calls have spent host time since the
 * last reset (process-wide, every thread). calls / zeroCopyCalls: calls, and those whose every buffer
 * was pinned (one kernel over PCIe, no copies); registeredHits / pointerQueries: buffers classified
 * from the registration cache / by a runtime pointer query; classifyNs: classifying the buffers;
 * copyNs: host staging copies; launchNs: queuing kernels (and, on the runtime-copy pipeline, its
 * asynchronous copies); waitNs: waiting for the stream or a slot's kernel (kernel run time included).
 * reset != 0 zeroes the counters after reading them.
 */
typedef struct {
  uint64_t calls, zeroCopyCalls, registeredHits, pointerQueries;
  uint64_t classifyNs, copyNs, launchNs, waitNs;
} nexrHostPathStats;
NEXR_API nexrResult_t nexrGetHostPathStats(nexrHostPathStats* stats, int reset);

/*
 * nexrHostToDevRedOp — replaces hostToDevRedOp (reference src/enqueue.cc:2185-2278) for the
 * built-in ops: encodes (op, datatype, nRanks) into the device op and its 64-bit argument
 * (Min/Max xormask, Avg: integer nRanks<<1|signed or float 1/nRanks bit pattern). A user-created op
 * (its `default:` row, :2266-2275) is nexrInvalidArgument here: such ops belong to a communicator and are
 * resolved by the ring library's table (nexrRingRedOpCreatePreMulSum, include/nexr_ring.h).
 */
NEXR_API nexrResult_t nexrHostToDevRedOp(nexrDevRedOpFull* opFull, int op, int datatype, int nRanks);

/*
 * nexrLaunchOneRank — replaces ncclLaunchOneRank (reference src/device/onerank.cc:48-83,
 * declared src/include/device.h:1171): the nRanks == 1 all-reduce. Non-PreMulSum ops are a
 * stream-ordered copy (skipped when dst == src); PreMulSum runs a K=1 reduce-copy with the
 * scalar pre-op and postOp (onerank.cc:14-45), the scalar loaded from device memory when
 * redOp.scalarArgIsPtr.
 */
NEXR_API nexrResult_t nexrLaunchOneRank(void* dst, const void* src, size_t nElts, nexrDevRedOpFull redOp,
                                        int datatype, nexrStream_t stream);

/* One LL-protocol FIFO line — identical layout to union ncclLLFifoLine (reference
 * src/include/device.h:695-708): 8 data bytes split in two 32-bit halves, each followed by the
 * step flag; a line is valid when flag1 == flag2 == the expected flag. */
typedef struct {
  uint32_t data1, flag1, data2, flag2;
} nexrLLFifoLine;

/*
 * nexrReduceCopyLL — one step of the LL protocol's reduce-copy, LLGenericOp<RECV, SEND, SrcBuf,
 * DstBuf> (reference src/device/prims_ll.h:218-283), with the step's FIFO slots resolved by the
 * caller: recvLines[i] / sendLines[i] point at the peer's slot (recvPtr(i)/sendPtr(i), :38-41) and
 * recvFlags[i] / sendFlags[i] are NCCL_LL_FLAG(step+1) (:42-43). Per 8-byte data line:
 *   d = src (x redOpArg when srcIsInput and the op is PreMulSum: applyPreOp(redOp, ·))
 *   d = nRecv ? (src ? op(peer0, d) : peer0) : d;  d = op(peer_i, d) for i >= 1   (peer FIRST)
 *   d = postOp ? d / divisor : d                                                  (SumPostDiv)
 *   sendLines[i] = {lo32(d), flag_i, hi32(d), flag_i};  dst = d  (valid elements only)
 * Recv lines are polled until both flags match (system-scope loads), for at most timeoutUs
 * (0 = 1 s); a line that never becomes valid sets *status = 1 (status: optional device/host-mapped
 * word) and its outputs are left unwritten — the kernel never hangs. A poll that keeps failing also
 * reads *status every 64 tries and gives up when it is non-zero (another step timed out, or the
 * caller wrote it to abort: checkAbort, primitives.h:142-156). src/dst are any-aligned device
 * pointers (nullable: at least one input and one output); line buffers must be 16-B aligned.
 *
 * Flag wrap: the caller resolves the flags and owns the credits, so it also owns the reference's slot
 * cleanup (incSend, prims_ll.h:85-93). On a send step s that cleans under its flag rule
 * ((s & cleanMask) == cleanMask, nexrLLFlagRule below) the contract is: queue nexrReduceCopyLL, then
 * nexrLLCleanSlot(nSend, sendLines, sendFlags, ceil(nElts*size/8), slotLines, stream) on the same
 * stream, before the step is published. A step with nElts == 0 on a cleaning step still cleans.
 */
NEXR_API nexrResult_t nexrReduceCopyLL(const void* src, int srcIsInput, int nRecv, const void* const* recvLines,
                                       const uint32_t* recvFlags, void* dst, int nSend, void* const* sendLines,
                                       const uint32_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                       uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                       nexrStream_t stream);

/*
 * nexrReduceCopyLL128 — one step of the LL128 protocol's reduce-copy, GenericOp +
 * recvReduceSendCopy (reference src/device/prims_ll128.h:184-331), the step's slots resolved by the
 * caller (recvPtr(i)/sendPtr(i), flags = step+1 as 64-bit words, :45-50). Wire format: 2 KiB slices
 * of sixteen 128-B lines carrying 1920 data bytes; word 15 of every line is the flag; user 16-B
 * chunk ix = g*32 - 4*(g/2) + w - (g%2)*(w/8) of a slice sits at wire words 64g + 2w (+1) for
 * w % 8 != 7, and the w % 8 == 7 chunks are split over words 64g + 2w of g and g+1 (loadRegsBegin/
 * loadRegsFinish/storeRegs :86-174) — byte-identical to the reference's warp-32 layout. Arithmetic,
 * peer-first operand order, status/timeout and pointer rules as nexrReduceCopyLL; wire buffers must
 * be 16-B aligned and hold ceil(nElts*size/1920) slices.
 *
 * Hand-off contract. The kernel accepts a line's data units from the same load that returned the line's
 * flag, and the producing kernel stores a line's data units and its flag unit in one instruction. A line
 * has ONE flag per 128 bytes and only 16-byte granules are observed untorn on gfx950 (the reference leans
 * on NVIDIA's 128-byte warp store, :186-204, :278-285), so a consumer that polls a slot while its
 * producer writes it could accept a line whose flag unit is new and another unit still old. The
 * consumer's kernel must therefore not START before its producer's kernel has COMPLETED (stream order,
 * an event, or a host wait; the ring's host sequencing does the last). Hand-off between kernels that run
 * at the same time is what nexrReduceCopyLL128StepsGroup is for.
 */
NEXR_API nexrResult_t nexrReduceCopyLL128(const void* src, int srcIsInput, int nRecv, const void* const* recvWire,
                                          const uint64_t* recvFlags, void* dst, int nSend, void* const* sendWire,
                                          const uint64_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                          uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                          nexrStream_t stream);

/*
 * nexrReduceCopyLLSteps — a run of LL steps of ONE Primitives (one rank's connections of one
 * channel) in as few launches as the steps allow, with the protocol's credits on the device: the
 * LLGenericOp calls of a schedule (reference src/device/prims_ll.h:249-318) together with their
 * waitSend / postRecv (:55-83), which the single-step nexrReduceCopyLL leaves to its caller.
 *
 * Every step of the run uses the same connections: nRecv receive FIFOs (steps with recv = 1 read all
 * of them, as LLGenericOp<RECV=1> does) and nSend send FIFOs, each nSlots (NCCL_STEPS) slots of
 * slotBytes. recvStep[i] / sendStep[i] are the connection's step counters at the first step of the
 * run (the flags follow: NCCL_LL_FLAG(step + 1), :42-43); each recv / send step advances them by one.
 * Credits live in device memory, one 8-byte word per wave at a 16-B stride, NEXR_LL_HEAD_BYTES per
 * connection (zeroed when the connection is made): the receiver stores its step count into its
 * connection's head words once it has read a step (postRecv), and a sender writes a slot only when
 * the head words of the connection it sends into show the step NCCL_STEPS earlier read (waitSend).
 * Both ends of a connection must therefore run their steps through this call (one wave of the
 * receiver's launch frees exactly the lines one wave of the sender's launch writes: both derive the
 * same grid from slotBytes). At the start of each launch the receiver stores recvStep into its
 * head words, so a connection may switch to this call after steps run by nexrReduceCopyLL once those
 * have completed.
 *
 * Element arithmetic, operand order, postOp, status and timeout as nexrReduceCopyLL, per step; user
 * offsets in elements of `datatype` (srcBuf / dstBuf: 0 input, 1 output, -1 none). The steps run as if
 * one at a time in order: where a step reads or writes user bytes an earlier step of the same launch
 * wrote or read at a different element position, the library starts a new launch. A step whose line
 * never arrives (or whose credit never comes) within timeoutUs sets *status = 1 and ends its
 * wave's run, and a non-zero *status ends the others' polls early (as nexrReduceCopyLL); the launch
 * never hangs. Launches are stream-ordered; the call returns after
 * queueing them. The runs on both ends of a connection must be able to run at once: streams on
 * hardware queues of their own (HIP shares its GPU_MAX_HW_QUEUES queues among streams and runs one
 * queue's kernels one after the other; a stream made by hipExtStreamCreateWithCUMask has its own), and
 * grids that fit the GPU together (one workgroup of 256 lanes per line tile of a slot, at most 64).
 */
#define NEXR_LL_STEPS_MAX_PEERS 3
#define NEXR_LL_HEAD_BYTES 4096
typedef struct {
  int64_t srcIx, dstIx; /* element offsets into the user buffer srcBuf / dstBuf */
  uint32_t nElts;       /* elements this step moves (0: the step only advances the counters) */
  uint8_t recv, send;   /* RECV / SEND of LLGenericOp */
  int8_t srcBuf, dstBuf;/* 0 input, 1 output, -1 none */
  uint8_t postOp;
  uint8_t pad[7];
} nexrLLStep;           /* 32 bytes */
typedef struct {
  const void* input;
  void* output;
  int nRecv, nSend;
  const void* recvFifo[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t* recvHead[NEXR_LL_STEPS_MAX_PEERS];       /* this rank's receive connections' head words */
  uint64_t recvStep[NEXR_LL_STEPS_MAX_PEERS];
  void* sendFifo[NEXR_LL_STEPS_MAX_PEERS];
  const uint64_t* sendHead[NEXR_LL_STEPS_MAX_PEERS]; /* the receivers' head words of the send connections */
  uint64_t sendStep[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t slotBytes; /* bytes per FIFO slot, every connection (16-B multiple) */
  uint32_t nSlots;    /* NCCL_STEPS: 1 .. INT_MAX (more: nexrInvalidArgument) */
  uint32_t pad;
} nexrLLConnSet;
NEXR_API nexrResult_t nexrReduceCopyLLSteps(const nexrLLConnSet* conns, const nexrLLStep* steps, int nSteps,
                                            int datatype, int devRedOp, uint64_t redOpArg, uint32_t* status,
                                            uint32_t timeoutUs, nexrStream_t stream);

/*
 * The LL flag rule and the flag-wrap slot cleanup (reference src/device/prims_ll.h:85-93 incSend,
 * src/include/device.h:719-728). An LL line is accepted when both its 32-bit flags equal
 * NCCL_LL_FLAG(step + 1), so a line written once and never overwritten would match again when the flag
 * comes round. The reference therefore rewrites, on every send step s with (s & NCCL_LL_CLEAN_MASK) ==
 * NCCL_LL_CLEAN_MASK, every line of the step's slot behind the step's data as {0, flag, 0, flag}: with
 * the production mask 0x7ffffff8 and NCCL_STEPS = 8 that is eight steps in a row every 2^31 steps, one
 * per slot. The rule is a parameter here so that the cleanup can be exercised without 2^31 steps of
 * traffic: {0x100, 0x78} is the reference's compile-time TEST_LL_CLEANUP mode.
 *
 * A rule is valid for nSlots slots when flagMax is 0 or a power of two, cleanMask != 0,
 * cleanMask % nSlots == 0 (the reference's static_assert) and the cleaning period
 * 2^(msb(cleanMask) + 1) is at most the flag period (flagMax, or 2^32 when flagMax == 0). NULL is the
 * production rule {0, 0x7ffffff8}. An invalid rule returns nexrInvalidArgument before any launch.
 */
typedef struct {
  uint32_t flagMax;   /* 0: NCCL_LL_FLAG(a) = (uint32_t)a;  else NCCL_LL_FLAG(a) = a % flagMax */
  uint32_t cleanMask; /* NCCL_LL_CLEAN_MASK: a send step s cleans when (s & cleanMask) == cleanMask */
} nexrLLFlagRule;

/*
 * nexrReduceCopyLLStepsRule — nexrReduceCopyLLSteps with the flag rule given (nexrReduceCopyLLSteps is
 * this call with rule = NULL, the production rule). The flags of every step come from the rule applied
 * to the 64-bit step counters, and on a cleaning send step the launch also writes lines
 * [ceil(nElts*size/8), slotBytes/16) of the step's slot of EVERY send connection as {0, flag, 0, flag}
 * (the reference calls incSend for every send), each line by the wave that owns it under the run's
 * credit map, after that wave's waitSend. A cleaning step with nElts == 0 cleans the whole slot. The
 * library ends a launch at every cleaning step and the kernel cleans behind its last step, so the
 * other steps carry no cost for it.
 */
NEXR_API nexrResult_t nexrReduceCopyLLStepsRule(const nexrLLConnSet* conns, const nexrLLStep* steps, int nSteps,
                                                int datatype, int devRedOp, uint64_t redOpArg,
                                                const nexrLLFlagRule* rule, uint32_t* status, uint32_t timeoutUs,
                                                nexrStream_t stream);

/*
 * nexrReduceCopyLLStepsGroup — the runs of nMembers Primitives (1..NEXR_LL_GROUP_MAX_MEMBERS: e.g. every
 * rank of a ring that lives on one GPU, times its channels) in the same launches on ONE stream. Member m
 * runs steps[m][0..nSteps[m]) on conns[m] exactly as nexrReduceCopyLLStepsRule would (the same argument
 * checks, reduction semantics, flags, credits and cleanup), but both ends of a connection between two
 * members sit in one grid (workgroup b runs member b / G as its workgroup b % G, G derived from slotBytes
 * as in nexrReduceCopyLLSteps), so the call needs no stream per member, no hardware queue of its own and
 * no assumption that separate kernels are scheduled together. slotBytes and nSlots must be equal for all
 * members (else nexrInvalidArgument). All members report into the one `status` word: a member that times
 * out ends the others' polls, and the launch never hangs.
 *
 * Launch cuts. A launch carries at most 96 steps of a member and, per member, ends where
 * nexrReduceCopyLLSteps would end it: before a step that touches user bytes an earlier step of the
 * launch touched at another element position, and behind a cleaning send step. A cut applies to every
 * member at the same step index (a member's part of a launch may be empty); user-range conflicts are
 * looked for within a member, not between members. All launches go on `stream`, in order.
 *
 * Dry run. Before any device call the library walks every launch on the host: connections whose FIFO
 * pointer is one member's send FIFO and another member's receive FIFO are internal (the sender's
 * sendStep must not be behind the receiver's recvStep), and their data and credit counters are stepped
 * round-robin through the launch's step lists from sendStep / recvStep; one-ended connections (the
 * peer runs elsewhere, through any of the LL steps calls) count as always ready. If a launch cannot
 * finish with what it and the launches before it produce — it would wait for a step of a later launch,
 * which starts only behind it — the call returns nexrInvalidUsage and launches nothing. Schedules where
 * step k of a member needs only steps <= k of its peers (the five ring collectives) always pass.
 *
 * Co-residency. nMembers * G workgroups must be resident at once: at most
 * hipOccupancyMaxActiveBlocksPerMultiprocessor(kernel, 256 lanes) x the device's CUs, else
 * nexrInvalidUsage (nothing launched).
 *
 * Workspace. Caller-owned device memory, 8-byte aligned, that holds the launches' parameter tables (one
 * block per member per launch; they do not fit the kernel-argument segment). The library fills one
 * DISTINCT region per launch of the call, so no table is written while a queued launch may read it: a
 * call that needs more launches than workspaceBytes holds regions for returns nexrInvalidArgument before
 * any device call. nexrLLGroupWorkspaceBytes(nMembers) is the size for NEXR_LL_GROUP_LAUNCHES launches
 * (768 steps per member when nothing cuts); a region is that size / NEXR_LL_GROUP_LAUNCHES, and any
 * larger workspace serves proportionally more launches (a call never needs more launches than its
 * longest step list has steps). The tables reach the device by ONE hipMemcpyAsync on `stream` from
 * pageable host memory, which the runtime stages before it returns, so nothing of the caller's arrays is
 * read after the call returns; the copy and the launches are stream-ordered. The caller must leave the
 * workspace alone (and not pass it to a call on another stream) until `stream` has passed the call; a
 * later call on the SAME stream may reuse it at once, its copy being ordered behind the earlier launches.
 */
#define NEXR_LL_GROUP_MAX_MEMBERS 32
#define NEXR_LL_GROUP_LAUNCHES 8
NEXR_API nexrResult_t nexrLLGroupWorkspaceBytes(int nMembers, size_t* bytes);
NEXR_API nexrResult_t nexrReduceCopyLLStepsGroup(int nMembers, const nexrLLConnSet* conns,
                                                 const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                 int devRedOp, uint64_t redOpArg, const nexrLLFlagRule* rule,
                                                 uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                 size_t workspaceBytes, nexrStream_t stream);

/*
 * nexrReduceCopyLL128StepsGroup — LL128 step lists of nMembers Primitives (1..NEXR_LL_GROUP_MAX_MEMBERS)
 * in the same launches on ONE stream: nexrReduceCopyLLStepsGroup for the LL128 wire (reference
 * src/device/prims_ll128.h: GenericOp :294-331, waitSend / postRecv :58-75, loadRegsBegin / recvReduceSendCopy
 * :86-292). nexrLLConnSet and nexrLLStep are used unchanged, read for LL128:
 *   - slotBytes is a multiple of 2048: a slot holds slotBytes / 2048 wire slices of 16 lines x 128 bytes,
 *     1920 data bytes each, so a step's nElts may fill at most slotBytes / 2048 * 1920 bytes (more:
 *     nexrInvalidArgument). The wire is byte-identical to nexrReduceCopyLL128's and the reference's: user
 *     chunk map ix(g, wid), the 64-bit flag in word 15 of every line;
 *   - the flags are recvStep + 1 / sendStep + 1 as 64-bit values, counted per connection from the
 *     counters in conns[m]; there is no flag rule and no cleanup (the reference cleans nothing for LL128).
 * Element arithmetic, peer-first operand order, pre/post op, the reduction semantics (nccl / fork /
 * shipped) and the datatypes and ops accepted are those of nexrReduceCopyLL128, per step.
 *
 * The hand-off is ordered by construction, which is what lets a consumer poll a slot while its producer
 * writes it (the single step nexrReduceCopyLL128 does not allow that, see there). A producing wave stores
 * the seven data units of each of its lines for every send connection, waits until those stores have
 * completed, and only then stores the lines' flag units (8 data bytes and the flag in one 16-byte
 * store); a consuming wave polls the flag units and, once every flag is there, loads the lines AGAIN, so
 * that a data unit enters the arithmetic only from a load issued after the flag had been seen. Credits
 * are per wave on the device head words (NEXR_LL_HEAD_BYTES per connection, zeroed before the first
 * use), as in nexrReduceCopyLLSteps: tile t (4 KiB of wire) of every step belongs to workgroup t % G,
 * G = min(64, ceil(slotBytes / 4096)), on both ends. A line or a credit that never comes within timeoutUs
 * sets *status = 1 and ends its wave's run; a non-zero *status ends the other polls early; the launch
 * never hangs.
 *
 * Everything else is nexrReduceCopyLLStepsGroup's, by the same host code: the argument checks, equal
 * slotBytes / nSlots across members, the launch cuts (96 steps, a member's user-range conflict, applied
 * to all members at one step index), the dry run (nexrInvalidUsage when a launch cannot finish), the
 * co-residency check (nexrInvalidUsage) and the workspace rules, sized by nexrLLGroupWorkspaceBytes (the
 * table entries are the same). All of these return before any device call. A group of ONE member with
 * one-ended connections is the "run" form: its peer's launch must then be able to run at the same time
 * (a stream on a hardware queue of its own, grids resident together), which is the caller's business.
 */
NEXR_API nexrResult_t nexrReduceCopyLL128StepsGroup(int nMembers, const nexrLLConnSet* conns,
                                                    const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                    int devRedOp, uint64_t redOpArg, uint32_t* status,
                                                    uint32_t timeoutUs, void* workspace, size_t workspaceBytes,
                                                    nexrStream_t stream);

/*
 * nexrReduceCopySimpleStepsGroup — SIMPLE step lists of nMembers Primitives (1..NEXR_LL_GROUP_MAX_MEMBERS)
 * in the same launches on ONE stream: the group call for the protocol whose data carries no flags
 * (reference src/device/prims_simple.h: genericOp :190-330, waitPeer / postPeer :111-188). nexrLLStep is
 * used unchanged; one record is ONE SLICE of genericOp:
 *   - srcs = [user src if srcBuf != -1, then the slot of every receive connection when recv], dsts = [user
 *     dst if dstBuf != -1, then the slot of every send connection when send]; acc = srcs[0], the USER source
 *     first (nexrReduceCopy's order, not the LL calls' peer-first one); the PreMulSum pre-op applies to
 *     source 0 only when srcBuf == 0 (the user input), postOp as in the record. Element arithmetic, the
 *     reduction semantics (nccl / fork / shipped) and the datatypes and ops accepted are nexrReduceCopy's
 *     (fp8 is refused, as in the LL calls);
 *   - a connection's slot is fifo + (step % nSlots) * slotBytes; a slice may fill stepPerSlice consecutive
 *     slots (nElts * size <= slotBytes * stepPerSlice, else nexrInvalidArgument), and a recv or send record
 *     advances the counters by stepPerSlice. A record with nElts == 0 only advances and posts;
 *   - stepPerSlice >= 1, nSlots % stepPerSlice == 0, and every recvStep / sendStep is a multiple of
 *     stepPerSlice (a slice never wraps the FIFO), else nexrInvalidArgument; slotBytes (a 16-B multiple),
 *     nSlots and stepPerSlice are equal across members; FIFOs are 16-B aligned, user buffers at any
 *     alignment; workgroupsPerMember is 0..NEXR_SIMPLE_GROUP_MAX_GRID.
 *
 * Credits are per WORKGROUP, in device memory: a connection has a tail block and a head block of
 * NEXR_SIMPLE_CREDIT_BYTES each (8-byte aligned, zeroed before the first use), one 8-byte word per workgroup
 * at a 16-B stride. Tile t of every slice, bytes [t * 4096, t * 4096 + 4096) from the slice's start, belongs
 * to workgroup t % G on both ends of a connection; G is workgroupsPerMember, or for 0
 * min(256, ceil(slotBytes * stepPerSlice / 4096)). Word w of the tail block says how far the sender's
 * workgroup w has published, word w of the head block how far the receiver's workgroup w has released: a
 * sender's workgroup writes a slot only when head[w] + nSlots >= sendStep + stepPerSlice, a receiver's reads
 * only when tail[w] >= recvStep + stepPerSlice. A workgroup that owns no tile of a slice neither waits nor
 * is waited for on it; it still advances and posts. At the start of a launch a member stores recvStep into
 * its head words and sendStep into its tail words, so a connection may come from host-sequenced steps that
 * have completed. The tail is published behind a release fence and read in front of an acquire fence, both
 * at system scope. A tail or a head that never comes within timeoutUs (0: one second) sets
 * *status = 1 and ends its workgroup's run; a non-zero *status ends the other polls early; the launch never
 * hangs.
 *
 * The host side is nexrReduceCopyLLStepsGroup's, by the same code: the launch cuts (96 records, a member's
 * user-range conflict, applied to all members at one index), the dry run (nexrInvalidUsage when a launch
 * cannot finish; the credit test is sendStep + stepPerSlice - nSlots <= head), the co-residency check
 * (nMembers * G workgroups resident at once, else nexrInvalidUsage) and the workspace rules, sized by
 * nexrSimpleGroupWorkspaceBytes for NEXR_LL_GROUP_LAUNCHES launches (too small: nexrInvalidArgument). All of
 * these return before any device call. A group of ONE member with one-ended connections is the "run" form.
 */
#define NEXR_SIMPLE_CREDIT_BYTES 4096   /* per connection and direction: one 8-byte word per workgroup at a 16-B stride */
#define NEXR_SIMPLE_GROUP_MAX_GRID 256  /* workgroups per member at most: NEXR_SIMPLE_CREDIT_BYTES / 16 */
typedef struct {
  const void* input;
  void* output;
  int nRecv, nSend;
  const void* recvFifo[NEXR_LL_STEPS_MAX_PEERS];
  const uint64_t* recvTail[NEXR_LL_STEPS_MAX_PEERS]; /* written by the sender */
  uint64_t* recvHead[NEXR_LL_STEPS_MAX_PEERS];       /* written by this member */
  uint64_t recvStep[NEXR_LL_STEPS_MAX_PEERS];
  void* sendFifo[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t* sendTail[NEXR_LL_STEPS_MAX_PEERS];       /* written by this member */
  const uint64_t* sendHead[NEXR_LL_STEPS_MAX_PEERS]; /* written by the receiver */
  uint64_t sendStep[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t slotBytes;    /* stepSize: bytes per FIFO step, a 16-B multiple */
  uint32_t nSlots;       /* NCCL_STEPS */
  uint32_t stepPerSlice; /* StepPerSlice of the collective's ProtoSimple: every step record is one slice */
} nexrSimpleConnSet;
NEXR_API nexrResult_t nexrSimpleGroupWorkspaceBytes(int nMembers, size_t* bytes);
NEXR_API nexrResult_t nexrReduceCopySimpleStepsGroup(int nMembers, const nexrSimpleConnSet* conns,
                                                     const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                     int devRedOp, uint64_t redOpArg, int workgroupsPerMember,
                                                     uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                     size_t workspaceBytes, nexrStream_t stream);

/*
 * nexrReduceCopySimpleStepsGroupDirect — nexrReduceCopySimpleStepsGroup with DirectWrite connections
 * (reference src/device/prims_simple.h:148-164, :258-269): a sender writes into the RECEIVING member's output
 * buffer at the record's dstIx instead of a FIFO slot, and the receiver reads its own output there. `direct`
 * is one nexrSimpleDirectSet per member, or NULL; with NULL the call IS nexrReduceCopySimpleStepsGroup (the
 * same kernels, tables and workspace size).
 *
 * A record permits direct ends in nexrLLStep.pad[0] (every other call ignores the pad bytes):
 * NEXR_SIMPLE_DIRECT_RECV is DirectRecv1, NEXR_SIMPLE_DIRECT_SEND DirectSend1 of the reference's genericOp.
 * An end is direct only when the record's bit AND the connection's entry say so. Per record, on a member
 * with output O and element size `size`:
 *   - send connection j with sendDirect[j] != NULL: the destination is sendDirect[j] + dstIx * size, at any
 *     alignment, instead of the slot (dstIx is read also when dstBuf == -1);
 *   - the receive connection with recvDirect[0] != 0: the source is O + dstIx * size instead of the slot. Only
 *     one receive may be direct: a member with any recvDirect set needs nRecv == 1 and a non-NULL output
 *     (else nexrInvalidArgument);
 *   - a direct receive with srcBuf == -1 and dstBuf == 1 has its source and its user destination at the same
 *     bytes: nothing is stored to O. If the record sends, that one source is copied to the send destinations
 *     bit for bit (no pre-op, no post-op); if not, the record moves no data: it waits, advances and posts;
 *   - everything else is nexrReduceCopySimpleStepsGroup's: the operand order [user src, receive...], the
 *     pre-op, the post-op, the reduction semantics. The bytes every member ends with equal the FIFO path's.
 * Tiles, credits, the timeout and the status word are unchanged (tile t of a slice counts from the slice's
 * start address, which both ends compute alike); the tail and head words after a direct run equal those of
 * the same lists through FIFOs, and a direct slice writes no FIFO byte.
 *
 * Host side, before any device call: the checks of nexrReduceCopySimpleStepsGroup; a connection between two
 * members (one's sendFifo is the other's recvFifo) must be direct on both ends or on neither, with
 * sendDirect equal to the receiver's output (else nexrInvalidArgument); one-ended connections are trusted,
 * as is the room behind sendDirect. For the launch cuts a direct source is a read of the member's output at
 * dstIx; a direct destination belongs to no member (the connection's credits order it). The workspace is
 * sized by nexrSimpleGroupDirectWorkspaceBytes when direct != NULL.
 */
#define NEXR_SIMPLE_DIRECT_RECV 1u
#define NEXR_SIMPLE_DIRECT_SEND 2u
typedef struct {
  void*   sendDirect[NEXR_LL_STEPS_MAX_PEERS]; /* element 0 of the RECEIVING member's output buffer; NULL: this connection uses its FIFO */
  uint8_t recvDirect[NEXR_LL_STEPS_MAX_PEERS]; /* 1: the sender of receive connection i writes into THIS member's output */
  uint8_t pad[5];
} nexrSimpleDirectSet;
NEXR_API nexrResult_t nexrSimpleGroupDirectWorkspaceBytes(int nMembers, size_t* bytes);
NEXR_API nexrResult_t nexrReduceCopySimpleStepsGroupDirect(int nMembers, const nexrSimpleConnSet* conns,
                                                           const nexrLLStep* const* steps, const int* nSteps,
                                                           int datatype, int devRedOp, uint64_t redOpArg,
                                                           int workgroupsPerMember, const nexrSimpleDirectSet* direct,
                                                           uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                           size_t workspaceBytes, nexrStream_t stream);

/*
 * nexrSymAllReduce — the symmetric all-reduce ncclSymRun_AllReduce_RSxLD_AGxST (reference
 * src/device/symmetric/all_reduce.hh:6-276) of nRanks ranks that live on ONE GPU, as one launch: peer loads
 * and peer stores only, no FIFO, no credits, no fences, n reads and n writes per element. inputs[r] /
 * outputs[r] are rank r's buffers of nElts elements (the reference's symmetric windows; here plain device
 * memory). Additions only: the ABI stays 0.3. Its siblings ncclSymRun_ReduceScatter_LD and
 * ncclSymRun_AllGather_ST are nexrSymReduceScatter and nexrSymAllGather below, and the family's LL members
 * (AllReduce_AGxLL_R, ReduceScatter_LL, AllGather_LL) the nexrSymLL* calls behind them. The all-reduce's
 * multicast kernels (…MC, …LLMC) and the multicast forms (…MC) of the symmetric
 * ReduceScatter_LD / AllGather_ST are not built.
 *
 * Ownership rule. n = nRanks (2..NEXR_SYM_MAX_RANKS), B = nBlocks (1..64, ncclSymMaxBlocks,
 * src/include/symmetric.h:8; 0 means 1), esz = 2 or 4, nBytes = nElts * esz. The geometry comes from rank 0's
 * pointers, as in the reference ("move to rank 0", all_reduce.hh:199-209): A = inputs[0] mod 16,
 * D = (inputs[0] - outputs[0]) mod 16. With pre = min((16 - A) mod 16, nBytes) and cursor = pre (:207-209):
 *   pass 1 (:213-228), only when D = 0: c1 = floor((nBytes - cursor) / 8192), c1 -= c1 mod (n * B); the
 *     c1 * 8192 bytes from cursor are cut into 2048-byte pieces, piece i owned by rank i mod n;
 *     cursor += c1 * 8192;
 *   pass 2 (:230-245), when esz = 4 or D mod 4 = 0: c2 = floor((nBytes - cursor) / 2048),
 *     c2 -= c2 mod (n * B); the c2 * 2048 bytes from cursor are cut into 512-byte pieces, piece i owned by
 *     rank i mod n; cursor += c2 * 2048;
 *   ends (:249-251, :134-135): the pre / esz leading elements followed by the (nBytes - cursor) / esz trailing
 *     ones, numbered e = 0, 1, ...; element e is owned by rank floor(e / 32) mod n.
 * (A piece is one iteration of a reference warp, 4 packs x 32 lanes x 16 or 4 bytes, and the warps are
 * numbered by rank first, :262-267, so iteration i is rank i mod n's whatever the block size.) B fixes only
 * the pass boundaries: it is the reference's CTA count, which it derives from a bandwidth model of NVIDIA
 * hardware (src/symmetric.cc:105-289) that is not restated; the caller passes B, and the launch geometry here
 * does not depend on it.
 *
 * An element owned by rank o is acc = inputs[o], then acc = acc + inputs[(o + j) mod n] for j = 1..n-1 in that
 * order, the accumulator as first operand (allreduceDeep :23-81, allreduceEnds :134-169), the additions in
 * fp32 for all three datatypes (ncclSymAccumType, symmetric/primitives.hh:426-434): fp16 and bf16 are
 * widened exactly and rounded back once at the end, round-to-nearest-even, every NaN to 0x7fff; fp32
 * denormals are kept and nothing is contracted. The result is stored to outputs[o], outputs[o + 1], ..., all n
 * outputs (:83-104, :171-188). This fold order and accumulator type are no nexrReduceCopy call's.
 *
 * Barriers. The reference kernel arrives at a cross-rank barrier when it starts and waits for it before its
 * first peer load, and arrives (release) and waits again when it ends (all_reduce.hh:269-275), so that no
 * rank reads a peer's input before that peer has reached the collective and no rank leaves while a peer still
 * reads its input or writes its output. With every rank on one GPU both are the stream's order: the launch
 * starts after everything queued on `stream` before it and completes before anything queued behind it.
 *
 * datatype is nexrFloat32, nexrFloat16 or nexrBfloat16 and devRedOp nexrDevSum (symmetric/generate.py:48-50;
 * redOpArg is ignored). In place (outputs[r] == inputs[r]) is allowed, and any output may equal any input
 * whole, because every element is read by its one owner before it is written; partial overlap is undefined.
 * Under nexrSemanticsShipped every add returns its first operand, so each element is its owner's input
 * through the two casts; nccl and fork are identical here. Stream-ordered: one launch, no workspace, and
 * nothing of the caller's arrays is read after the call returns. nElts == 0 succeeds without a launch.
 * nexrInvalidArgument, before any device call: null arrays or entries, nRanks outside 2..64, nBlocks outside
 * 0..64, another datatype or op, a pointer not aligned to esz.
 */
#define NEXR_SYM_MAX_RANKS 64
NEXR_API nexrResult_t nexrSymAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                       size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                       int nBlocks, nexrStream_t stream);

/*
 * nexrSymReduceScatter — the symmetric reduce-scatter ncclSymRun_ReduceScatter_LD (reference
 * src/device/symmetric/reduce_scatter.hh:6-241) of nRanks ranks that live on ONE GPU, as one launch: peer
 * loads only, one store per element. inputs[r] holds nRanks * nElts elements, outputs[r] holds nElts.
 * Additions only: the ABI stays 0.3.
 *
 * Rule. For every rank r and element e: acc = inputs[r][r * nElts + e], then
 * acc = acc + inputs[(r + j) mod n][r * nElts + e] for j = 1..n-1 in that order, the accumulator as first
 * operand (reduceDeep :23-89, reduceEnds :118-157; the kernel hands rank r its chunk as
 * input + prim.rank*args->nElts, :237). Chunk r is folded from rank r's own input, not rank 0's. The sum is in
 * fp32 for all three datatypes (ncclSymAccumType, symmetric/primitives.hh:426-434): fp16 and bf16 are widened
 * exactly and rounded back once at the end, round-to-nearest-even, every NaN to 0x7fff; fp32 denormals are
 * kept and nothing is contracted. The result goes to outputs[r][e] only. No ring or tree entry point folds in
 * this order or with this accumulator (the ring's reduce-scatter is rank-ordered through FIFOs with one
 * rounding per step).
 *
 * No ownership map. The reference's pass ladder and CTA count (reduce_scatter.hh:160-220: 16-byte packs,
 * 4-byte packs, element-wise ends, chunks rounded to n * nBlocks) only spread one rank's elements over that
 * rank's own warps; every path folds in the same order with the same accumulator. So no output byte depends
 * on alignment or on nBlocks: the entry takes no nBlocks, and the device layout (every chunk cut from its byte
 * 0 into 2048-byte pieces, 16-byte packs and single elements) is free.
 *
 * Barriers. The reference kernel arrives at a cross-rank barrier when it starts, waits for it before its first
 * peer load, and arrives and waits again when it ends (reduce_scatter.hh:234-240). With every rank on one GPU
 * both are the stream's order, as for nexrSymAllReduce.
 *
 * datatype is nexrFloat32, nexrFloat16 or nexrBfloat16 and devRedOp nexrDevSum (symmetric/generate.py:48-50;
 * redOpArg is ignored). Aliasing: outputs[r] may be chunk r of any rank's input, that is the address
 * inputs[s] + r * nElts * esz for some s (NCCL's in-place form is s = r): such an element is read by the one
 * lane that writes it, before the write. Any other overlap of an output with an input or another output is
 * undefined, as in the reference. Under nexrSemanticsShipped every add returns its first operand, so the
 * result is rank r's own chunk through the two casts; nccl and fork are identical here. Stream-ordered: one
 * launch, no workspace, and nothing of the caller's arrays is read after the call returns. nElts == 0
 * succeeds without a launch. nexrInvalidArgument, before any device call: null arrays or entries, nRanks
 * outside 2..NEXR_SYM_MAX_RANKS, another datatype or op, a pointer not aligned to esz, nRanks * nElts * esz
 * overflowing size_t.
 */
NEXR_API nexrResult_t nexrSymReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                           size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                           nexrStream_t stream);

/*
 * nexrSymAllGather — the symmetric all-gather ncclSymRun_AllGather_ST (reference
 * src/device/symmetric/all_gather.hh:5-177) of nRanks ranks that live on ONE GPU, as one launch: one load
 * and n peer stores per byte. inputs[r] holds nBytes bytes, outputs[s] holds nRanks * nBytes.
 *
 * Rule. outputs[s][r * nBytes + b] = inputs[r][b] for every s, r and b: a bit copy at any byte alignment, so
 * there is no datatype (the reference runs it on char, :173). When inputs[r] == outputs[r] + r * nBytes, rank
 * r skips its own output: the reference's inPlace (:105, :33, :81), decided per rank. Any other overlap of an
 * input with an output is undefined. The reference's pass ladder (:101-158) only picks the width of a copy,
 * so the device layout is free here too. Its barriers (:170-176) are the stream's order.
 *
 * Stream-ordered: one launch, no workspace. nBytes == 0 succeeds without a launch. nexrInvalidArgument,
 * before any device call: null arrays or entries, nRanks outside 2..NEXR_SYM_MAX_RANKS, nRanks * nBytes
 * overflowing size_t.
 */
NEXR_API nexrResult_t nexrSymAllGather(int nRanks, const void* const* inputs, void* const* outputs, size_t nBytes,
                                       nexrStream_t stream);

/*
 * nexrSymLLAllReduce, nexrSymLLReduceScatter, nexrSymLLAllGather — the LL members of the symmetric family,
 * ncclSymRun_AllReduce_AGxLL_R (reference src/device/symmetric/all_reduce.hh:356-428),
 * ncclSymRun_ReduceScatter_LL (reduce_scatter.hh:320-388) and ncclSymRun_AllGather_LL (all_gather.hh:256-363),
 * which the reference runs for small messages, of nRanks ranks that live on ONE GPU, each as one launch. They
 * sit on ncclSymPrims' sendLL / bcastLL / recvLL / recvReduceLL / endLL (symmetric/primitives.hh:212-377): data
 * travels as 16-byte lines {lo, flag, hi, flag} through per-rank windows. Additions only: the ABI stays 0.3.
 * Opt-in like their siblings: nothing chooses them automatically. n = nRanks (2..NEXR_SYM_MAX_RANKS), esz = 2
 * or 4.
 *
 * AllReduce (AGxLL_R). inputs[r] / outputs[r] hold nElts elements. For every element e and every rank s:
 * acc = inputs[0][e], then acc = acc + inputs[j][e] for j = 1..n-1 in rank order, the accumulator as first
 * operand (recvReduceLL folds rank 0 first on every rank, primitives.hh:349-377), in fp32 for fp32, fp16 and
 * bf16 (ncclSymAccumType, primitives.hh:425-434): fp16 and bf16 are widened exactly and rounded back once,
 * round-to-nearest-even, every NaN to 0x7fff; fp32 denormals are kept and nothing is contracted. The result is
 * stored to outputs[s][e]. Beyond 8 ranks the reference folds in groups of 8; the order stays rank order. There
 * is no ownership map: no byte depends on alignment, on nBlocks or on the 8-byte pack. These are not
 * nexrSymAllReduce's bytes (owner first) and not the ring's or tree's (a rounding per step).
 *
 * ReduceScatter (LL). inputs[r] holds n * nElts elements, outputs[r] holds nElts. outputs[r][e] is the same
 * rank-0-first fp32 fold of inputs[j][r * nElts + e], j = 0..n-1. For chunks r >= 1 and n >= 3 these are not
 * nexrSymReduceScatter's bytes (chunk r from rank r on).
 *
 * AllGather (LL). inputs[r] holds nBytes bytes, outputs[s] holds n * nBytes.
 * outputs[s][r * nBytes + b] = inputs[r][b]: a bit copy at any byte alignment, without a datatype.
 *
 * Common. datatype is nexrFloat32, nexrFloat16 or nexrBfloat16 and devRedOp nexrDevSum (symmetric/generate.py;
 * redOpArg is ignored). Under nexrSemanticsShipped every add returns its first operand: the all-reduce is
 * rank 0's input through the two casts and the reduce-scatter chunk r of rank 0's input; nccl and fork are
 * identical here. Allowed aliasing: outputs[r] == inputs[r] (all-reduce), outputs[r] == inputs[r] +
 * r * nElts * esz (reduce-scatter), inputs[r] == outputs[r] + r * nBytes (all-gather): a lane loads its pack
 * before it stores it. Any other overlap is undefined. The reference's 8-byte-aligned and element-wise paths
 * (all_reduce.hh:369-423) only pick access widths: the entries take any element-aligned pointers, the
 * all-gather any byte-aligned ones.
 *
 * Windows. windows[r] is rank r's window: caller-owned device memory, 16-byte aligned, at least
 * nexrSymLLWindowBytes(nRanks, B) bytes, zeroed once before its first use, touched by nothing else.
 *   header    uint32_t llEpoch[64] (as ncclSymDevBase, src/include/symmetric.h:20-31), padded to
 *             NEXR_SYM_LL_HEADER_BYTES: word b is block b's stored epoch, the next flag minus 2;
 *   lines     from byte NEXR_SYM_LL_HEADER_BYTES: per block b two buffers, for even and odd flags, of
 *             n * NEXR_SYM_LL_ROUND_PACKS 16-byte lines each; block b's start at line
 *             2 * b * n * NEXR_SYM_LL_ROUND_PACKS, whatever B is. Nothing else about the line area is fixed.
 * A group of windows serves ONE nRanks (the line layout depends on it; nBlocks may change from call to call):
 * zero all of them before using them with another. All windows of a group carry equal epoch words. Zeroing ALL windows of a group (header and lines) resets it;
 * the words may also be set by plain copies while every window's lines are consistent with them (zero lines
 * are: flags 0 and 1 never occur, so a zeroed window matches nothing).
 *
 * Protocol. B = nBlocks (1..64, 0 means 1). The grid is n * B teams of one workgroup, team w = (rank w mod n,
 * block w / n). With P = ceil(bytes / 8) 8-byte packs (bytes = nElts * esz, the chunk's for the
 * reduce-scatter, nBytes for the all-gather), team (r, b) takes floor(P / B) packs plus one for b < P mod B,
 * consecutive from block 0 on, in rounds of at most NEXR_SYM_LL_ROUND_PACKS packs. Round k of a call uses flag
 * f = llEpoch[b] + 2 + k in 32 bits, and after 0xffffffff the next flag is 2; when the team ends it stores
 * (next flag - 2) back. A block without packs runs no round and leaves its word. In a round the team puts pack
 * t of its round as the line {lo, f, hi, f} into slot r * NEXR_SYM_LL_ROUND_PACKS + t of block b's parity-f
 * buffer in EVERY window, its own included (the reduce-scatter: the pack of chunk s into window s), then polls
 * the n lines of each of its packs in its own window, and ends the round with a team barrier (endLL): no lane
 * of a rank sends round k + 1 before its team has read round k, which is what makes two buffers enough. In a
 * round whose flag is >= 0xfffffffe the team zeroes that parity's whole buffer after its reads, with
 * system-coherent 16-byte stores that every wave drains before the barrier, so that no line of the cycle that
 * ends can satisfy a poll of the next.
 *
 * status and timeoutUs are nexrReduceCopyLL's: a line that does not arrive within timeoutUs (0 = 1 s) sets
 * *status = 1 (optional device or host-mapped word); a non-zero *status ends the other polls early. The team
 * of a poll that gave up skips its later polls and stores but reaches all its barriers: the launch always
 * ends. After a non-zero status the outputs and the windows are undefined and the caller zeroes ALL windows
 * before the next call.
 *
 * Stream-ordered, one launch. A count of 0 succeeds without a launch and leaves the epoch words alone.
 * nexrInvalidArgument, before any device call: null arrays or entries; nRanks outside
 * 2..NEXR_SYM_MAX_RANKS; another datatype or op; an input or output not aligned to esz or a window not aligned
 * to 16; nBlocks outside 0..64; windowBytes below nexrSymLLWindowBytes(nRanks, B); nElts * esz or nBytes (for
 * the reduce-scatter n * nElts * esz too) at or above 2^31 (the reference's int nElts: these are the
 * small-message kernels); an overflowing product. nexrInvalidUsage, without a launch: the grid of n * B
 * workgroups is not resident as a whole on the current device (teams poll each other, so a queued team could
 * keep resident ones waiting until their timeouts).
 */
#define NEXR_SYM_LL_HEADER_BYTES 256 /* uint32_t llEpoch[64] */
#define NEXR_SYM_LL_ROUND_PACKS 256  /* 8-byte packs per team and round */
#define NEXR_SYM_LL_MAX_BLOCKS 64
NEXR_API nexrResult_t nexrSymLLWindowBytes(int nRanks, int maxBlocks, size_t* bytes);
NEXR_API nexrResult_t nexrSymLLAllReduce(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                         int datatype, int devRedOp, uint64_t redOpArg, void* const* windows,
                                         size_t windowBytes, int nBlocks, uint32_t* status, uint32_t timeoutUs,
                                         nexrStream_t stream);
NEXR_API nexrResult_t nexrSymLLReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                             size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                             void* const* windows, size_t windowBytes, int nBlocks,
                                             uint32_t* status, uint32_t timeoutUs, nexrStream_t stream);
NEXR_API nexrResult_t nexrSymLLAllGather(int nRanks, const void* const* inputs, void* const* outputs, size_t nBytes,
                                         void* const* windows, size_t windowBytes, int nBlocks, uint32_t* status,
                                         uint32_t timeoutUs, nexrStream_t stream);

/*
 * nexrFlatAllReduce, nexrFlatReduceScatter, nexrFlatReduce — the RING all-reduce, reduce-scatter and reduce
 * (runRing, reference src/device/all_reduce.h:12-84, reduce_scatter.h:12-52, reduce.h:12-50) of nRanks ranks
 * that live on ONE GPU, each as one launch that writes exactly the bytes the ring's chain of reduce-copy steps
 * writes: for all ten datatypes (not fp8), all five device ops and both operand orders. Where the nexrSym*
 * calls fold owner first in fp32 with one rounding, these run the ring's own chain, one step and one rounding
 * per rank, in registers: peer loads and stores only, no FIFO, no credit, no poll between workgroups, so a
 * launch cannot stall on residency. Additions only: the ABI stays 0.3. n = nRanks (2..NEXR_SYM_MAX_RANKS),
 * esz = the datatype's size.
 *
 * Rule for one element. The element has a start rank s (per collective, below).
 *   v = in[s]. Under nexrDevPreMulSum it passes through the pre-op (times the scalar redOpArg encodes) and
 *     then through the canonicalisation that a K = 1 reduce-copy with a pre-op applies (fp16 / bf16: every NaN
 *     to 0x7fff). Without a pre-op it is a bit copy: NaN payloads survive (directSend / sendInput).
 *   For j = 1..n-1, r = (s + j) mod n: v = one reduce-copy step of {in[r] through the pre-op, v}.
 *     userFirst != 0 (SIMPLE): in[r] is the first operand (srcs[0] is the user input, prims_simple.h:238-242;
 *     nexrReduceCopy's order). userFirst == 0 (LL, LL128): v is the first operand (prims_ll.h:251-258,
 *     prims_ll128.h:214-219). The step's own fp16 / bf16 rounding and NaN canonicalisation follow EVERY step,
 *     not the chain as a whole; nothing is contracted.
 *   The nexrDevSumPostDiv post-op runs on the last step only (postOp of the chain's last rank).
 *
 * AllReduce. inputs[r] / outputs[r] hold nElts elements. parts[k] = {offset, count, chunkCount} in elements
 * are the channels' views of the buffer (ncclCollCbdPart, src/include/device.h:946-970, with the channel's
 * chunkCount of calcCollChunking, src/enqueue.cc:1993-2062); they tile [0, nElts) in ascending order. For
 * element i of a part (runRingAllReduce, all_reduce.h:12-84):
 *   j = i - offset, loop = n * chunkCount, L = floor(j / loop), rem = count - L * loop,
 *   cc = rem < loop ? alignUp(divUp(rem, n), 16 / esz) : chunkCount, c = floor((j - L * loop) / cc),
 *   s = (c + 1) mod n.
 * The result goes to all n outputs. Every offset and chunkCount is a multiple of 16 / esz, so every chunk
 * boundary lies a multiple of 16 bytes from element 0.
 *
 * ReduceScatter. inputs[r] holds n * nElts elements, outputs[r] holds nElts. Element e of chunk d reads
 * inputs[*][d * nElts + e] with s = (d + 1) mod n (reduce_scatter.h:12-52: the chain ends at rank d); the
 * result goes to outputs[d][e] only.
 *
 * Reduce. inputs[r] and output hold nElts elements. s = (root + 1) mod n (reduce.h:12-50); the result goes
 * to output, the root's, only: nothing else is written.
 *
 * Semantics. nexrSemanticsFork runs signed Min / Max on the unsigned type, as every other call. Under
 * nexrSemanticsShipped every reduce returns its first operand without pre-op or post-op, as in the SIMPLE
 * group kernel: the result is a bit copy of in[(s + n - 1) mod n] with userFirst and of in[s] without.
 *
 * Aliasing. Any output may equal any input whole (the one lane that writes an element has read it from every
 * input first); the reduce-scatter's outputs[r] may be chunk r of any input (inputs[t] + r * nElts * esz).
 * Any other overlap is undefined. Pointers need element alignment only.
 *
 * Stream-ordered and one launch each; nothing of the caller's arrays is read after the call returns. Only an
 * all-reduce with more than NEXR_FLAT_INLINE_PARTS parts takes a workspace: stream-ordered memory of the
 * current device that short launches ahead of the one fill with the parts and that is freed behind it.
 * nElts == 0 succeeds without a launch. nexrInvalidArgument, before any device call: null arrays or entries;
 * nRanks outside 2..NEXR_SYM_MAX_RANKS; an fp8 or unknown datatype; an op that the datatype does not have
 * (nexrDevSumPostDiv on a float; a signed one-byte divide by a divisor that truncates to 0); root outside
 * 0..n-1; a pointer not aligned to esz; parts that do not tile [0, nElts) in ascending order or hold an empty
 * part; a part offset or chunkCount that is zero (chunkCount) or not a multiple of 16 / esz; an overflowing
 * product (nElts * esz, n * nElts * esz, n * chunkCount).
 */
typedef struct {
  uint64_t offset;      /* first element of the channel's part */
  uint64_t count;       /* its elements */
  uint64_t chunkCount;  /* the channel's chunk in elements */
} nexrFlatPart;
#define NEXR_FLAT_INLINE_PARTS 120
NEXR_API nexrResult_t nexrFlatAllReduce(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                        int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                        const nexrFlatPart* parts, int nParts, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatReduce(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                                     int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                     nexrStream_t stream);

/*
 * nexrFlatTreeAllReduce, nexrFlatBroadcast — the TREE all-reduce (runTreeSplit, reference
 * src/device/all_reduce.h:150-230) and the broadcast (broadcast.h:12-58) of nRanks ranks on ONE GPU, each as
 * one launch that writes the bytes the FIFO collective writes. Datatypes, ops, operand orders, alignment,
 * aliasing, semantics and stream order as nexrFlatAllReduce above; additions only, the ABI stays 0.3.
 *
 * Trees. trees[t][r] = {up, down[3]} are the links of rank r in tree t (nTrees 1 or 2: the double binary tree's
 * two); -1 is no link, children are packed first. parts[k] = {offset, count, tree} in elements tile [0, nElts)
 * in ascending order (the channels' parts); every offset is a multiple of 16 / esz, so no 16-byte pack holds
 * elements of two parts. The chunking inside a part does not enter the result.
 *
 * Rule for one element of a part whose tree is t. Every rank r has a value(r), ONE reduce-copy step over its
 * own input and its children's values in down[] order:
 *   acc = in[r] through the pre-op (nexrDevPreMulSum: times the scalar; the rank's own input only).
 *   For each child k in down[] order: acc = op(acc, value(k)) when userFirst != 0 (SIMPLE: srcs[0] is the user
 *     input, a left fold), acc = op(value(k), acc) when userFirst == 0 (LL, LL128: the peer is the first
 *     operand, prims_ll.h:251-258). Every op rounds to the datatype; the step ends with the fp16 / bf16 NaN
 *     canonicalisation. Nothing is contracted.
 *   A leaf's value is the K = 1 step: a bit copy without a pre-op (NaN payloads survive), the product and that
 *     step's canonicalisation with one.
 *   The root's step ends with the nexrDevSumPostDiv post-op; its value goes to all n outputs.
 * Under nexrSemanticsShipped every reduce returns its first operand without pre-op or post-op: the result is a
 * bit copy of the root's input with userFirst, and without it of the input of the leaf reached from the root
 * through every rank's LAST child.
 *
 * How it runs. Each tree is compiled on the host into a program of one-byte instructions (LEAF r, JOIN r,
 * PUSH, MERGE; at most 3n - 2) that the kernel interprets in registers: from the root, down[0]'s value first,
 * then the rank's own input, then for every further child the accumulator is saved, the child evaluated and
 * the two merged. A program may keep at most NEXR_FLAT_TREE_SLOTS values alive at once (the accumulator and the
 * saved ones); every topology the ring library builds up to 64 ranks needs 6 at the most.
 *
 * nexrFlatBroadcast copies nBytes from input (the root's) to every outputs[r] whose address differs from it:
 * a bit copy at any byte alignment. An output may equal the input whole; any other overlap is undefined.
 *
 * nElts == 0 / nBytes == 0 succeed without a launch. Only an all-reduce with more than
 * NEXR_FLAT_TREE_INLINE_PARTS parts takes a (stream-ordered) workspace. nexrInvalidArgument, before any device
 * call: everything nexrFlatAllReduce refuses for its buffers, datatype, op and sizes; nTrees outside 1..2 or a
 * null tree; a part naming a missing tree; parts that do not tile [0, nElts) in ascending order, hold an empty
 * part or begin off a multiple of 16 / esz; links that are not ONE spanning tree (exactly one root, every up
 * matched by its parent's down and every down by its child's up, no cycle, no rank out of range, children
 * packed first); a program that needs more than NEXR_FLAT_TREE_SLOTS live values.
 */
typedef struct {
  int up;      /* the parent, -1 at the root */
  int down[3]; /* the children in fold order, packed first, -1 for none */
} nexrFlatTreeLinks;
typedef struct {
  uint64_t offset; /* first element of the channel's part */
  uint64_t count;  /* its elements */
  uint32_t tree;   /* index into trees */
  uint32_t pad;    /* 0 */
} nexrFlatTreePart;
#define NEXR_FLAT_TREE_SLOTS 8
#define NEXR_FLAT_TREE_INLINE_PARTS 96
NEXR_API nexrResult_t nexrFlatTreeAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, const nexrFlatTreeLinks* const* trees, int nTrees,
                                            const nexrFlatTreePart* parts, int nParts, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatBroadcast(int nRanks, const void* input, void* const* outputs, size_t nBytes,
                                        nexrStream_t stream);

/*
 * nexrFlatAllReducePreMul, nexrFlatReduceScatterPreMul, nexrFlatReducePreMul, nexrFlatTreeAllReducePreMul —
 * nexrFlatAllReduce, nexrFlatReduceScatter, nexrFlatReduce and nexrFlatTreeAllReduce under nexrDevPreMulSum with
 * a scalar PER RANK: what a user-created PreMulSum op needs (ncclRedOpCreatePreMulSum, reference
 * src/enqueue.cc:2447-2487; include/nexr_ring.h has the op table). The per-element rules are the ones stated
 * above for nexrDevPreMulSum with "times the scalar" read as "times scalars[r] for rank r's input": indexed by the
 * RANK whose input it is, whatever that rank's place in the chain or in the tree's program. Additions only: the
 * ABI stays 0.3.
 *
 * scalars[r], r < nRanks: the raw bits of one element of `datatype` (the low bytes), or, with scalarsArePtrs !=
 * 0, the device address of that element (element-aligned, readable on the current device). A device-resident
 * scalar is read by the kernel itself, with no host read and no synchronisation: it holds whatever the stream
 * wrote before the launch, and a replay of a captured graph sees the value current at the replay.
 *
 * Everything else is the plain entry's: the argument checks (plus nexrInvalidArgument for a null `scalars`, and
 * with scalarsArePtrs for a null or misaligned entry), aliasing, alignment, stream order, graph capture, the
 * parts, the trees, the semantics modes. Under nexrSemanticsShipped the pre-op returns its input, so the result
 * is the plain entry's bit copy and does not depend on the scalars (they are not read). The kernels are separate
 * instances, one per datatype; their argument block holds the n scalars in the room of inline parts, so an
 * all-reduce takes the stream-ordered workspace beyond NEXR_FLAT_PREMUL_INLINE_PARTS parts and a tree all-reduce
 * beyond NEXR_FLAT_TREE_PREMUL_INLINE_PARTS (the ring library's most is 64, one per channel).
 */
#define NEXR_FLAT_PREMUL_INLINE_PARTS 96
#define NEXR_FLAT_TREE_PREMUL_INLINE_PARTS 64
NEXR_API nexrResult_t nexrFlatAllReducePreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                              size_t nElts, int datatype, const uint64_t* scalars,
                                              int scalarsArePtrs, int userFirst, const nexrFlatPart* parts,
                                              int nParts, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatReduceScatterPreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                                  size_t nElts, int datatype, const uint64_t* scalars,
                                                  int scalarsArePtrs, int userFirst, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatReducePreMul(int nRanks, const void* const* inputs, void* output, int root,
                                           size_t nElts, int datatype, const uint64_t* scalars, int scalarsArePtrs,
                                           int userFirst, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatTreeAllReducePreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                                  size_t nElts, int datatype, const uint64_t* scalars,
                                                  int scalarsArePtrs, int userFirst,
                                                  const nexrFlatTreeLinks* const* trees, int nTrees,
                                                  const nexrFlatTreePart* parts, int nParts, nexrStream_t stream);

/*
 * nexrFlatHostAllReduce, nexrFlatHostReduceScatter, nexrFlatHostReduce, nexrFlatHostTreeAllReduce,
 * nexrFlatHostBroadcast, nexrFlatHostAllGather — the flat collectives over HOST memory: the arguments, the
 * per-element rules, the bytes, the aliasing rules and the argument checks (nexrInvalidArgument before any
 * device call) of nexrFlatAllReduce, nexrFlatReduceScatter, nexrFlatReduce, nexrFlatTreeAllReduce,
 * nexrFlatBroadcast and nexrSymAllGather, with every buffer in host memory. The call returns when the outputs
 * are complete, as nexrReduceCopyHost does. Additions only: the ABI stays 0.3.
 *
 * Every distinct (address, length) among the buffers is classified once, as nexrReduceCopyHost classifies a
 * buffer: the registration cache (nexrHostRegister, nexrHostMemAlloc) without a runtime call, else the
 * runtime's pointer query, trusted only when the whole buffer lies inside the pinned range it reports; a
 * buffer that begins inside a pinned range and runs past its end is staged and copied in pieces.
 * NEXR_HOST_ZERO_COPY=0 stages everything. With every buffer pinned the call is ONE launch that reads and
 * writes the user buffers in place over the link, its grid capped at NEXR_HOST_GRID (32) workgroups. Otherwise
 * pageable inputs are copied into device memory before the launch and pageable outputs out of it behind the
 * launch; pinned buffers are still accessed in place; outputs that receive the same bytes (the all-reduces,
 * the broadcast, the all-gather) share one staged output. The ring and the tree all-reduce, the reduce and the
 * broadcast run calls of more than NEXR_FLAT_HOST_CHUNK_BYTES (read once per process, 32 MiB, cut to a
 * multiple of 2048) as a two-slot window pipeline: window w is copied in and launched while window w - 1 is
 * copied out on a second stream. The reduce-scatter and the all-gather stage whole.
 *
 * nexrGetFlatHostStats — diagnostics (process-wide, every thread) since the last reset: calls that reached
 * the classification; zeroCopyCalls: those with every buffer pinned; stagedBuffers: device slots that staged
 * calls used (one per distinct pageable input, one per distinct pageable output, or one for all pageable
 * outputs where they share); registeredHits / pointerQueries: distinct buffers classified from the
 * registration cache / by a runtime query; windows: launches (one per window; a zero-copy call is one).
 * reset != 0 zeroes the counters after reading them.
 */
typedef struct {
  uint64_t calls, zeroCopyCalls, stagedBuffers, registeredHits, pointerQueries, windows;
} nexrFlatHostStats;
NEXR_API nexrResult_t nexrFlatHostAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, const nexrFlatPart* parts, int nParts,
                                            nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatHostReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                                size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                                int userFirst, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatHostReduce(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                                         int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                         nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatHostTreeAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                                size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                                int userFirst, const nexrFlatTreeLinks* const* trees, int nTrees,
                                                const nexrFlatTreePart* parts, int nParts, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatHostBroadcast(int nRanks, const void* input, void* const* outputs, size_t nBytes,
                                            nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatHostAllGather(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nBytes, nexrStream_t stream);
NEXR_API nexrResult_t nexrGetFlatHostStats(nexrFlatHostStats* stats, int reset);

/*
 * nexrFlatGroup, nexrFlatGroupPlan — SEVERAL flat collectives as flat GROUP launches: what ncclGroupStart /
 * ncclGroupEnd fuse (reference src/group.cc:17, :90-96; tasks binned by (func, op, datatype),
 * src/enqueue.cc:374-385; several ncclDevWorkColl in one kernel, src/device/common.h:292-330). A single flat
 * call is its launch and its completion wait; a group pays them once for many works. Additions only: the ABI
 * stays 0.3. Device memory of the current device; PreMulSum with a scalar per rank, the tree all-reduce and
 * host memory are not grouped.
 *
 * works[i] is one call. coll NEXR_FLAT_GROUP_ALL_REDUCE / _REDUCE_SCATTER / _REDUCE: nexrFlatAllReduce /
 * nexrFlatReduceScatter / nexrFlatReduce with the work's datatype, devRedOp, redOpArg, root (reduce), inputs,
 * outputs (the reduce reads outputs[root] only), nElts, and parts / nParts (all-reduce). NEXR_FLAT_GROUP_COPY:
 * nElts BYTES from inputs[0] to outputs[0 .. nOutputs), as nexrFlatBroadcast copies (any byte alignment; an
 * output at the source's address is skipped); a broadcast is one such work, an all-gather n of them. nRanks and
 * userFirst hold for every reducing work.
 *
 * The result is the bytes the same works give when issued in array order through the single entries. The host
 * walks the works in order and keeps one open launch per (datatype, devRedOp, min-or-max) and one for copies; a
 * work joins its open launch. Two works conflict when a write range of one intersects a read or a write range
 * of the other (byte ranges, half-open, as long as the entry's contract says: an all-reduce reads and writes
 * nElts * esz bytes per buffer, a reduce-scatter reads n * nElts * esz, a reduce writes its root's output only);
 * aliasing inside one work stays as the single entry defines it. A work that conflicts with a work of ANY open
 * launch first closes all open launches, which are queued in the order they were opened; at the end the
 * remaining ones are queued in that order. launchOf[i] (may be NULL) receives the launch of work i in queue
 * order, -1 for a work with nElts == 0, which costs nothing.
 *
 * A launch runs the table of its works (flat_group_kernel / flat_group_copy_kernel): records with pointers for
 * nRanks ranks only and the parts in a pool behind them. A table that fits NEXR_FLAT_GROUP_INLINE_BYTES rides
 * in the kernel arguments, and the launch takes no workspace; a longer one goes by value, in short fill
 * launches ahead of the launch, into stream-ordered memory that is freed behind it. Nothing of the caller's
 * arrays is read after the call returns, so the call can be captured into a graph. maxWorkgroups caps every
 * launch's grid (waves then stride over the items); 0: a wave per 2048-byte piece over the launch's summed
 * pieces, four waves per workgroup. nWorks == 0 succeeds without a launch.
 *
 * info (may be NULL): works placed in a launch, launches, fill launches, cuts, the sum of the tables' bytes and of
 * the launches' workgroups. nexrFlatGroupPlan does the same validation and fills launchOf and info without any
 * device call.
 *
 * nexrInvalidArgument, before any device call: everything the single entry of a work refuses for its buffers,
 * datatype, op, root, sizes and parts; a null `works`; nWorks < 0; an unknown coll; nOutputs
 * outside 1..NEXR_SYM_MAX_RANKS or a null source or destination (copy); maxWorkgroups < 0.
 */
#define NEXR_FLAT_GROUP_ALL_REDUCE 0
#define NEXR_FLAT_GROUP_REDUCE_SCATTER 1
#define NEXR_FLAT_GROUP_REDUCE 2
#define NEXR_FLAT_GROUP_COPY 3
#define NEXR_FLAT_GROUP_INLINE_BYTES 3936 /* the longest table that rides in the kernel arguments */
#define NEXR_FLAT_GROUP_FILL_BYTES 3968   /* what one fill launch carries of a longer one */
typedef struct {
  int coll;                   /* NEXR_FLAT_GROUP_* */
  int datatype;               /* reducing works */
  int devRedOp;
  int root;                   /* reduce */
  uint64_t redOpArg;
  const void* const* inputs;  /* nRanks entries; copy: inputs[0] */
  void* const* outputs;       /* nRanks entries; copy: nOutputs */
  int nOutputs;               /* copy only */
  int nParts;                 /* all-reduce only */
  const nexrFlatPart* parts;
  size_t nElts;               /* copy: bytes */
} nexrFlatGroupWork;
typedef struct {
  int works;          /* works that went into a launch */
  int launches;       /* group launches */
  int fillLaunches;   /* launches that carry tables too long for the kernel arguments */
  int cuts;           /* conflicts that closed the open launches */
  uint64_t tableBytes;
  uint64_t workgroups;
} nexrFlatGroupInfo;
NEXR_API nexrResult_t nexrFlatGroup(int nRanks, const nexrFlatGroupWork* works, int nWorks, int userFirst,
                                    int maxWorkgroups, int* launchOf, nexrFlatGroupInfo* info, nexrStream_t stream);
NEXR_API nexrResult_t nexrFlatGroupPlan(int nRanks, const nexrFlatGroupWork* works, int nWorks, int userFirst,
                                        int maxWorkgroups, int* launchOf, nexrFlatGroupInfo* info);

/*
 * nexrLLCleanSlot — the cleanup for callers of the single-step nexrReduceCopyLL: writes lines
 * [firstLine, slotLines) of each of the nSend (<= NEXR_MAX_DSTS) slots sendLines[i] as
 * {0, sendFlags[i], 0, sendFlags[i]}, one 16-byte system-coherent store per line, stream-ordered.
 * sendLines[i] are the slot bases the step's nexrReduceCopyLL wrote to (non-NULL, 16-B aligned, else
 * nexrInvalidArgument); firstLine is the step's line count. firstLine >= slotLines is a successful no-op.
 */
NEXR_API nexrResult_t nexrLLCleanSlot(int nSend, void* const* sendLines, const uint32_t* sendFlags, size_t firstLine,
                                      size_t slotLines, nexrStream_t stream);

/*
 * Reduction semantics — which nex-nccl the library reproduces bit for bit. Process-wide, like an
 * NCCL parameter: the initial value comes from NEXR_SEMANTICS ("nccl", "fork" or "shipped"; default
 * "nccl"); nexrSetSemantics changes it for every later call (set it before the first call that
 * matters; calls already queued keep theirs). It applies to nexrReduceCopy, nexrReduceCopyBatch,
 * nexrReduceCopyMultiDevice, nexrReduceCopyHost, nexrLaunchOneRank, nexrReduceCopyLL and
 * nexrReduceCopyLL128, and so to every emulated collective built on them (include/nexr_ring.h).
 *   nexrSemanticsNccl     real arithmetic; Min/Max compared at the signedness of `datatype`
 *                         (upstream NCCL). The default.
 *   nexrSemanticsFork     the fork with SKIP_COMP removed: real arithmetic under the fork's own kernel
 *                         dispatch, where signed-integer Min/Max run on the unsigned kernel
 *                         (equivalent_primary, src/device/generate.py:128-136) whose FuncMinMax ignores
 *                         the sign xormask (reduce_kernel.h:59-65), so they compare as unsigned.
 *   nexrSemanticsShipped  the fork exactly as shipped: `#define SKIP_COMP` (reduce_kernel.h:432) makes
 *                         every ncclReduceScalar return its FIRST operand and the PreMulSum pre-op and
 *                         SumPostDiv post-op return their input (:434-539). reduceCopy then copies
 *                         srcs[0]'s bits to every destination; an LL / LL128 step (peer first) forwards
 *                         the last peer's data, or src when it has no peer.
 * Argument validation is the same in every mode.
 */
typedef enum {
  nexrSemanticsNccl = 0,
  nexrSemanticsFork = 1,
  nexrSemanticsShipped = 2,
  nexrNumSemantics = 3
} nexrSemantics_t;
NEXR_API nexrResult_t nexrSetSemantics(int semantics);
NEXR_API nexrResult_t nexrGetSemantics(int* semantics);

/*
 * nexrQueryLaunch — diagnostics: the launch nexrReduceCopy would make for these pointers and this
 * size (no GPU work, no device needed; the same validation as nexrReduceCopy with devRedOp = Sum). A
 * one-source call runs as a byte copy (the uint8 kernel), so its headElts and bodyPacks count bytes.
 * [0, headElts) and the tail are edge elements (headElts brings dsts[0] to a 128-B boundary when its
 * offset is a whole number of elements) and bodyPacks 16-B packs form the body, pack i being the 16
 * bytes at offset 16 i of every buffer. `unaligned` is 1 when the pointers share no 16-B phase: the
 * body then moves the misaligned buffers with unaligned 16-B accesses (ABI 0.2 dropped round 1's
 * always-zero `generic` field: `unaligned` now sits at offset 16). grid * block never exceeds 2^32 - 1 work items
 * (HIP's launch limit); larger calls grid-stride. policy: 0 plain, 1 non-temporal loads, 3
 * non-temporal loads and stores.
 */
typedef struct {
  uint32_t grid;
  int block;
  int packsPerLane;
  int policy;
  int unaligned;
  uint64_t headElts;
  uint64_t bodyPacks;
} nexrLaunchInfo;
NEXR_API nexrResult_t nexrQueryLaunch(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                      size_t nElts, int datatype, nexrLaunchInfo* info);

/* Diagnostics: how many streams nexrReduceCopyMultiDevice and how many staging rings
 * nexrReduceCopyHost have created in this process so far (device rings of the chunk pipeline plus
 * pinned rings of the large-call copy-team path; all pooled and reused, so the counts stop growing
 * once the pools are warm). Either pointer may be NULL. */
NEXR_API nexrResult_t nexrGetPoolStats(uint64_t* multiDeviceStreams, uint64_t* hostStagingRings);

/* Bytes per element of a datatype (reference ncclTypeSize), 0 if unknown. */
NEXR_API size_t nexrTypeSize(int datatype);

/* Human-readable string for a result code (reference ncclGetErrorString). */
NEXR_API const char* nexrGetErrorString(nexrResult_t result);

/* Packed version: major*10000 + minor*100 + patch. */
NEXR_API int nexrGetVersion(void);

/* Last HIP error recorded by this thread inside the library (0 if none) — diagnostics only. */
NEXR_API int nexrGetLastHipError(void);

#ifdef __cplusplus
}
#endif

#endif /* NEXR_H_ */
