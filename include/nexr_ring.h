/*
 * nexr_ring.h — CPU-emulated collectives that drive the reduce-copy ABI (include/nexr.h) from the
 * reference's own schedules: the caller side of the drop-in boundary.
 *
 * It restates, on host threads (one per emulated rank, two for a non-root tree rank, 1 channel):
 *   - runRing for ncclAllReduce (reference src/device/all_reduce.h:12-84), ncclReduceScatter
 *     (reduce_scatter.h:12-52), ncclAllGather (all_gather.h:12-66), ncclReduce (reduce.h:12-50) and
 *     ncclBroadcast (broadcast.h:12-58),
 *   - runTreeSplit for the tree ncclAllReduce (all_reduce.h:150-230) over the reference's tree
 *     topology: an intra-node chain (graph/connect.cc:51-61) whose node heads are joined by the
 *     double binary tree (graph/trees.cc:31-109, connect.cc:95-163),
 *   - Primitives::genericOp slicing and the reduceCopy call sites (src/device/prims_simple.h:190-330,
 *     directSend/directRecvReduceDirectSend/directRecvReduceCopyDirectSend/directRecvCopyDirectSend/
 *     directRecv :897-976),
 *   - the FIFO credit protocol of waitPeer/postPeer (prims_simple.h:111-188): NCCL_STEPS = 8 slots of
 *     buffBytes/8 per connection, head/tail step counters, StepPerSlice = 2, SlicePerChunk = 2
 *     (src/include/collectives.h:17-18),
 *   - or, with protocol = LL, LLGenericOp's one-step-per-call credits and line flags
 *     NCCL_LL_FLAG(step+1) (src/device/prims_ll.h:55-93, :218-283; chunk = stepSize/2,
 *     src/enqueue.cc:1997); with LL128, GenericOp's steps and 64-bit line flags step+1
 *     (src/device/prims_ll128.h:55-85, :294-331; chunk = stepSize*15/16, enqueue.cc:1998),
 *   - the host chunking for ring SIMPLE (src/enqueue.cc:1993-1996: chunkSize = stepSize * 4),
 *   - ncclLaunchOneRank for nRanks == 1 (src/device/onerank.cc:48-83),
 *   - op encoding through nexrHostToDevRedOp (src/enqueue.cc:2185-2278).
 * Every reduceCopy site calls a nexrReduceCopyFn — nexrReduceCopyHost (host memory) or
 * nexrReduceCopy + a wait for the step's completion (device memory) by default.
 *
 * Library: libnexr_ring.so (links libnexr.so). The schedules beyond SURVEY §8's rows — ncclSend /
 * ncclRecv and the device-resident forms — are declared in nexr_extras.h and built only into the
 * opt-in libnexr_extras.so (a superset of libnexr_ring.so; `make EXTRAS=1`).
 */
#ifndef NEXR_RING_H_
#define NEXR_RING_H_

#include "nexr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Same signature as nexrReduceCopy / nexrReduceCopyHost. */
typedef nexrResult_t (*nexrReduceCopyFn)(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                         size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                         int nPreOpSrcs, const uint64_t* preOpArgs, int postOp,
                                         nexrStream_t stream);

/* Same signature as nexrReduceCopyLL. */
typedef nexrResult_t (*nexrReduceCopyLLFn)(const void* src, int srcIsInput, int nRecv, const void* const* recvLines,
                                           const uint32_t* recvFlags, void* dst, int nSend, void* const* sendLines,
                                           const uint32_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                           uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                           nexrStream_t stream);

/* Same signature as nexrReduceCopyLL128. */
typedef nexrResult_t (*nexrReduceCopyLL128Fn)(const void* src, int srcIsInput, int nRecv, const void* const* recvWire,
                                              const uint64_t* recvFlags, void* dst, int nSend, void* const* sendWire,
                                              const uint64_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                              uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                              nexrStream_t stream);

typedef enum { nexrRingHostMemory = 0, nexrRingDeviceMemory = 1 } nexrRingMemMode_t;
/* The two protocols the emulated ring restates (the reference's NCCL_PROTO_SIMPLE / NCCL_PROTO_LL).
 * Numbered so that a zero-initialised config selects SIMPLE. */
typedef enum { nexrRingProtoSimple = 0, nexrRingProtoLL = 1, nexrRingProtoLL128 = 2 } nexrRingProto_t;

typedef struct {
  int nRanks;          /* emulated ranks (threads), >= 1 */
  size_t buffBytes;    /* per-connection buffer (NCCL_BUFFSIZE); 0 = the protocol default: 4 MiB
                          SIMPLE, 512 KiB LL, 4,915,200 B LL128 (src/init.cc:618-631) */
  int memMode;         /* nexrRingMemMode_t: where user buffers and FIFOs live */
  nexrReduceCopyFn fn; /* SIMPLE: NULL = nexrReduceCopyHost (host) / nexrReduceCopy (device) */
  int timeoutMs;       /* spin-wait bound per FIFO wait; 0 = 60000 */
  int protocol;        /* nexrRingProto_t (0 = SIMPLE) */
  nexrReduceCopyLLFn llFn; /* LL: NULL = nexrReduceCopyLL (device memory mode only) */
  nexrReduceCopyLL128Fn ll128Fn; /* LL128: NULL = nexrReduceCopyLL128 (device memory mode only) */
  int treeRanksPerNode; /* tree topology: ranks per emulated node (0 = all ranks on one node, i.e. a
                           chain); must divide nRanks. Node heads form the double binary tree */
  int treeIndex;        /* which tree of the double binary tree: 0 (the btree) or 1 (mirror/shift) */
  int nChannels;        /* channels (0 = 1, at most 64): every collective is split over them as the
                           reference's planner splits it (src/enqueue.cc:539-690); each channel has
                           its own links, FIFOs, streams and host threads and they run concurrently.
                           Like the reference's duplicated channels (graph/connect.cc:146-160), the
                           upper half of 2 or more channels uses the other tree of the double binary
                           tree. Send/Recv (extras) always uses channel 0 */
} nexrRingConfig;

typedef struct nexrRingComm* nexrRingComm_t;

/* Device mode: rank r uses HIP device r % deviceCount; FIFOs live on the receiving rank's device. */
NEXR_API nexrResult_t nexrRingCommCreate(nexrRingComm_t* comm, const nexrRingConfig* config);

/* ncclAllReduce over all emulated ranks at once: sendbuffs[r] / recvbuffs[r] are rank r's buffers
 * (host or device memory per memMode; in-place allowed). op is an ncclRedOp_t built-in or a handle of
 * nexrRingRedOpCreatePreMulSum (below). */
NEXR_API nexrResult_t nexrRingAllReduce(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                        size_t count, int datatype, int op);

/* ncclReduceScatter: rank r's sendbuffs[r] holds nRanks*recvcount elements; recvbuffs[r] receives the
 * reduction of every rank's segment r (recvcount elements). */
NEXR_API nexrResult_t nexrRingReduceScatter(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                            size_t recvcount, int datatype, int op);

/* ncclAllGather: recvbuffs[r] (nRanks*sendcount elements) receives every rank's sendbuff in rank order;
 * in place when sendbuffs[r] == recvbuffs[r] + r*sendcount elements. */
NEXR_API nexrResult_t nexrRingAllGather(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                        size_t sendcount, int datatype);

/* ncclReduce: recvbuffs[root] receives the reduction; other ranks' recvbuffs are not touched (may be NULL). */
NEXR_API nexrResult_t nexrRingReduce(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                     size_t count, int datatype, int op, int root);

/* ncclBroadcast: every recvbuffs[r] receives sendbuffs[root] (other ranks' sendbuffs may be NULL). */
NEXR_API nexrResult_t nexrRingBroadcast(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                        size_t count, int datatype, int root);

/* ncclAllReduce with NCCL_ALGO_TREE: runTreeSplit over the topology of config->treeRanksPerNode /
 * treeIndex. The reduce-up and broadcast-down halves of a non-root rank run on two threads, as the
 * reference splits a block's threads between them. */
NEXR_API nexrResult_t nexrTreeAllReduce(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                        size_t count, int datatype, int op);

/* ncclAllReduce as the reference's symmetric kernel RSxLD_AGxST (src/device/symmetric/all_reduce.hh:6-276):
 * ONE nexrSymAllReduce (include/nexr.h: the ownership rule, the owner-first fp32 fold, nBlocks) over every
 * rank's buffers on the communicator's first stream, then the wait the other collectives end with. No FIFO, no
 * step, no credit: it touches no connection and no step counter, so it mixes freely with ring and tree calls in
 * every mode, and it leaves nexrRingCommGetQueued as it was. Its bytes are NOT the ring's or the tree's: the
 * fold starts at the element's owner and accumulates in fp32 (one rounding for fp16 / bf16). It applies to thread
 * ranks, device memory and every rank on one GPU: anything else is nexrInvalidUsage; an op other than ncclSum,
 * a datatype other than float32 / float16 / bfloat16, nBlocks outside 0..64 or more than NEXR_SYM_MAX_RANKS
 * ranks is nexrInvalidArgument; one rank takes the one-rank path and count == 0 succeeds. In place allowed.
 * ReduceScatter_LD and AllGather_ST are the two entries below and the family's LL members the three
 * ...SymmetricLL entries behind them; the multicast symmetric kernels are not built. Measured on one
 * MI355X, a 4 MiB fp32 all-reduce per rank, p25-p75 of 20 calls on the host clock
 * (profiles/r14a_sym_all_reduce_probe.json): 0.018 / 0.026-0.031 /
 * 0.028-0.032 ms at 2 / 4 / 8 ranks against 0.140-0.191 / 0.335-0.377 / 1.030-1.119 for the host-sequenced ring
 * and 0.159-0.186 / 0.319-0.348 / 0.774-0.842 for the ring in group launches, the three alternated call by
 * call in one process, every call exact (tools/sym_all_reduce_probe.py). */
NEXR_API nexrResult_t nexrRingAllReduceSymmetric(nexrRingComm_t comm, const void* const* sendbuffs,
                                                 void* const* recvbuffs, size_t count, int datatype, int op,
                                                 int nBlocks);

/* ncclReduceScatter as the reference's symmetric kernel ReduceScatter_LD
 * (src/device/symmetric/reduce_scatter.hh:6-241): ONE nexrSymReduceScatter (include/nexr.h) over every rank's
 * buffers. sendbuffs[r] holds nRanks*recvcount elements, recvbuffs[r] receives chunk r folded from rank r's
 * own input on (then r + 1, ..., wrapping), in fp32 with one rounding for fp16 / bf16: NOT the ring's bytes,
 * whose fold is rank-ordered through FIFOs with a rounding per step. recvbuffs[r] may be chunk r of
 * sendbuffs[r] (ncclReduceScatter's in-place form). Everything else is as nexrRingAllReduceSymmetric states
 * it, through the same helper: the communicator's first stream and its wait, it touches no connection and no
 * step counter, it leaves nexrRingCommGetQueued as it was, thread ranks on one GPU with device memory or
 * anything else is nexrInvalidUsage, ncclSum of float32 / float16 / bfloat16 or nexrInvalidArgument, one rank
 * takes the one-rank path, recvcount == 0 succeeds. Never chosen automatically. Measured on one MI355X, a 4 MiB
 * fp32 input per rank, p25-p75 of 20 calls on the host clock (profiles/r15a_sym_rs_ag_probe.json):
 * 0.014-0.020 / 0.020-0.025 / 0.022-0.025 ms at 2 / 4 / 8 ranks against 0.128-0.160 / 0.260-0.285 /
 * 0.645-0.692 for the ring's own host-sequenced reduce-scatter and 0.129-0.160 / 0.243-0.254 / 0.516-0.560 in
 * group launches, alternated call by call in one process, every call exact (tools/sym_rs_ag_probe.py). */
NEXR_API nexrResult_t nexrRingReduceScatterSymmetric(nexrRingComm_t comm, const void* const* sendbuffs,
                                                     void* const* recvbuffs, size_t recvcount, int datatype,
                                                     int op);

/* ncclAllGather as the reference's symmetric kernel AllGather_ST (src/device/symmetric/all_gather.hh:5-177):
 * ONE nexrSymAllGather of sendcount * sizeof(datatype) bytes per rank. recvbuffs[s] (nRanks*sendcount
 * elements) receives every rank's sendbuff in rank order, a bit copy, so the bytes ARE the ring's all-gather's;
 * a rank with sendbuffs[r] == recvbuffs[r] + r*sendcount elements is in place and skips its own output.
 * Every datatype the ring's all-gather takes. The same helper and the same rules as the two calls above: it
 * touches no connection and no step counter, it leaves nexrRingCommGetQueued as it was, anything but thread
 * ranks on one GPU with device memory is nexrInvalidUsage, one rank takes the one-rank path, sendcount == 0
 * succeeds. Never chosen automatically (tools/sym_rs_ag_probe.py). */
NEXR_API nexrResult_t nexrRingAllGatherSymmetric(nexrRingComm_t comm, const void* const* sendbuffs,
                                                 void* const* recvbuffs, size_t sendcount, int datatype);

/* ncclAllReduce, ncclReduceScatter and ncclAllGather as the reference's symmetric LL kernels AllReduce_AGxLL_R,
 * ReduceScatter_LL and AllGather_LL (src/device/symmetric/all_reduce.hh:356-428, reduce_scatter.hh:320-388,
 * all_gather.hh:256-363), which it runs for small messages: ONE nexrSymLLAllReduce / nexrSymLLReduceScatter /
 * nexrSymLLAllGather (include/nexr.h: the rank-0-first fp32 fold, the windows, the protocol) over every rank's
 * buffers, through the helper of the three entries above, so their usage rules hold: the communicator's first
 * stream and its wait, thread ranks on one GPU with device memory or nexrInvalidUsage, ncclSum of float32 /
 * float16 / bfloat16 (the all-gather: every datatype the ring's takes) or nexrInvalidArgument, one rank takes
 * the one-rank path, a count of 0 succeeds, no connection and no step counter is touched and
 * nexrRingCommGetQueued stays as it was. The reduce-scatter's bytes are NOT nexrRingReduceScatterSymmetric's
 * (chunk r is folded from rank 0 on, not from rank r on) and the all-reduce's NOT nexrRingAllReduceSymmetric's
 * (rank 0 first, not owner first); neither are the ring's (fp32 accumulator, one rounding). In-place forms as
 * ncclAllReduce / ncclReduceScatter / ncclAllGather define them. The communicator allocates its n windows,
 * zeroed and sized for 16 blocks, on first use and frees them when it is destroyed: nBlocks is 0..16 (0 means
 * 1), anything else nexrInvalidArgument; a message of 2 GiB or more per rank is nexrInvalidArgument and a grid
 * that is not resident as a whole nexrInvalidUsage, as nexrSymLL* return them. The timeout is the
 * communicator's timeoutMs and the status word the one its LL paths report in: a call whose kernel reports a
 * timeout returns nexrInternalError, as those paths do, and the windows are zeroed again before the next
 * symmetric LL call. Never chosen automatically (tools/sym_ll_probe.py). */
NEXR_API nexrResult_t nexrRingAllReduceSymmetricLL(nexrRingComm_t comm, const void* const* sendbuffs,
                                                   void* const* recvbuffs, size_t count, int datatype, int op,
                                                   int nBlocks);
NEXR_API nexrResult_t nexrRingReduceScatterSymmetricLL(nexrRingComm_t comm, const void* const* sendbuffs,
                                                       void* const* recvbuffs, size_t recvcount, int datatype,
                                                       int op, int nBlocks);
NEXR_API nexrResult_t nexrRingAllGatherSymmetricLL(nexrRingComm_t comm, const void* const* sendbuffs,
                                                   void* const* recvbuffs, size_t sendcount, int datatype,
                                                   int nBlocks);

/* ncclAllReduce, ncclReduceScatter and ncclReduce of the RING, each as ONE launch with the ring's own bytes:
 * nexrFlatAllReduce / nexrFlatReduceScatter / nexrFlatReduce (include/nexr.h: the chain of one reduce-copy step
 * per rank, run in registers) over every rank's buffers. The argument lists are the plain calls' and so are
 * the results, byte for byte, for every datatype and op the plain calls take: the op is encoded as theirs
 * (Avg becomes PreMulSum or SumPostDiv), the all-reduce's chunks are this communicator's own (its channels'
 * parts and chunk counts for its protocol and FIFO size), and a SIMPLE communicator folds the user input
 * first where LL and LL128 fold the received partial first. Through the helper of the symmetric entries: the
 * communicator's first stream and its wait, thread ranks on one GPU with device memory or nexrInvalidUsage,
 * at most NEXR_SYM_MAX_RANKS ranks, one rank takes the one-rank path, a count of 0 succeeds; a reduce needs
 * recvbuffs[root] only and writes nothing else. No connection and no step counter is touched and
 * nexrRingCommGetQueued stays as it was, so flat and FIFO calls may alternate freely. In place as the plain
 * calls define it. Chosen for the plain calls only under nexrRingCommSetFlat. Measured numbers: DESIGN §8.7
 * (tools/flat_probe.py).
 *
 * Host memory. These entries, the three below and nexrRingCommSetFlat also take a HOST-memory communicator with
 * thread ranks, the SIMPLE protocol (the user input is a step's first operand), at most NEXR_SYM_MAX_RANKS
 * ranks and the library's own fn: the same parts, chunk counts, trees and op encoding go to the nexrFlatHost*
 * form of the entry (include/nexr.h), on the first rank's device and stream; pinned (registered, allocated)
 * user buffers are read and written in place over the link, pageable ones are staged, and the call returns
 * with the outputs complete. A host-memory communicator with a caller's fn or with LL or LL128 is
 * nexrInvalidUsage as before, and so is a process-rank communicator, from every one of these entries (the three
 * entries here and nexrTreeAllReduceFlat / nexrRingBroadcastFlat used to answer nexrInvalidArgument for one,
 * against this comment and against nexrRingCommSetFlat and nexrRingAllGatherFlat). Measured numbers: DESIGN §8.9 (tools/flat_host_probe.py). */
NEXR_API nexrResult_t nexrRingAllReduceFlat(nexrRingComm_t comm, const void* const* sendbuffs,
                                            void* const* recvbuffs, size_t count, int datatype, int op);
NEXR_API nexrResult_t nexrRingReduceScatterFlat(nexrRingComm_t comm, const void* const* sendbuffs,
                                                void* const* recvbuffs, size_t recvcount, int datatype, int op);
NEXR_API nexrResult_t nexrRingReduceFlat(nexrRingComm_t comm, const void* const* sendbuffs, void* const* recvbuffs,
                                         size_t count, int datatype, int op, int root);

/* The tree all-reduce, the broadcast and the all-gather as ONE launch each with the FIFO collective's own bytes,
 * through the same helper as the three entries above (thread ranks on one GPU with device memory or
 * nexrInvalidUsage, the communicator's first stream and its wait, one rank takes the one-rank path, a count of
 * 0 succeeds; no connection, no step counter and not nexrRingCommGetQueued's report is touched). The argument
 * lists are the plain calls'.
 *   nexrTreeAllReduceFlat: nexrFlatTreeAllReduce (include/nexr.h: every rank's one step over its own input and
 *     its children's values, interpreted in registers) with this communicator's channel parts, every
 *     channel's own tree (the upper half of 2+ channels runs the other tree of the double binary tree) and
 *     the protocol's operand order; the op is encoded as the plain call's.
 *   nexrRingBroadcastFlat: nexrFlatBroadcast of sendbuffs[root]; only that send buffer is needed.
 *   nexrRingAllGatherFlat: nexrSymAllGather under the flat name, whose bytes are the ring's already.
 * Measured numbers: DESIGN §8.8 (tools/flat_tree_probe.py). */
NEXR_API nexrResult_t nexrTreeAllReduceFlat(nexrRingComm_t comm, const void* const* sendbuffs,
                                            void* const* recvbuffs, size_t count, int datatype, int op);
NEXR_API nexrResult_t nexrRingBroadcastFlat(nexrRingComm_t comm, const void* const* sendbuffs,
                                            void* const* recvbuffs, size_t count, int datatype, int root);
NEXR_API nexrResult_t nexrRingAllGatherFlat(nexrRingComm_t comm, const void* const* sendbuffs,
                                            void* const* recvbuffs, size_t sendcount, int datatype);

/* Opt-in, off by default: which plain calls on an eligible communicator run as their flat entries above. `on`
 * is read as bits: NEXR_FLAT_RING (1) routes nexrRingAllReduce, nexrRingReduceScatter and nexrRingReduce;
 * NEXR_FLAT_TREE (2) routes nexrTreeAllReduce; NEXR_FLAT_COPIES (4) routes nexrRingAllGather and
 * nexrRingBroadcast. nexrRingCommGetQueued reports 4 after a routed call. Eligible: thread ranks, device
 * memory, every rank on one GPU, at most NEXR_SYM_MAX_RANKS ranks and the library's own fn (SIMPLE), llFn (LL)
 * or ll128Fn (LL128): a caller's function may compute anything; or thread ranks in HOST memory with SIMPLE and
 * the library's own fn (the host forms, see nexrRingAllReduceFlat above). On any other communicator, and for the calls
 * whose bit is not set, the calls run exactly as without the option. The results are the same bytes either way,
 * and the option may be changed between collectives and combined with the group options (a routed call ignores
 * them). With 0 nothing changes; with 1 exactly the three ring reductions are routed.
 *
 * nexrInvalidArgument for any other bit; nexrInvalidUsage for process-rank communicators and for host-memory
 * communicators with a caller's fn, LL or LL128. */
#define NEXR_FLAT_RING 1
#define NEXR_FLAT_TREE 2
#define NEXR_FLAT_COPIES 4
NEXR_API nexrResult_t nexrRingCommSetFlat(nexrRingComm_t comm, int on);

/*
 * nexrRingGroupStart, nexrRingGroupEnd — ncclGroupStart / ncclGroupEnd (reference src/nccl.h.in:472-504,
 * src/group.cc:17, :90-96) for a thread-rank communicator: the collectives called between the two are recorded
 * and run by the outermost nexrRingGroupEnd, and those that would run flat go out as flat GROUP launches
 * (nexrFlatGroup, include/nexr.h), so that many small calls pay one launch per kind and one completion wait. The
 * result is the bytes of the same calls made one by one in call order. Additions only: the ABI stays 0.3.
 *
 * Start and End nest by depth (ncclGroupDepth); an End without a Start and a process-rank communicator are
 * nexrInvalidUsage. While the depth is above 0 every collective entry of this header checks its arguments (the
 * communicator's state, datatype, op, root, null arrays and null buffers) and returns its error at once, without
 * recording the call; otherwise it copies its pointer arrays, records the call and returns nexrSuccess. Nothing
 * of the caller's arrays is read afterwards.
 *
 * The outermost End walks the recorded calls in order. A call becomes work records if it is a ring all-reduce,
 * reduce-scatter, reduce, all-gather or broadcast that would run flat (an explicit ...Flat entry, or a plain call
 * whose nexrRingCommSetFlat bit is set) on a device-memory communicator of 2 or more ranks on one GPU, without
 * per-rank scalars; runs of consecutive such calls go to ONE nexrFlatGroup call on the communicator's first
 * stream, each all-reduce with the channel parts it has alone (the reference's split of one channel set over the
 * tasks of a group, scheduleCollTasksToPlan, is not restated: it would change a grouped float all-reduce's
 * bytes). An all-gather is n copies, a broadcast one. Every other recorded call (the tree, a per-rank or
 * device-resident PreMulSum op, the symmetric entries, the FIFO paths, host memory, one rank) ends the run,
 * waits for what was queued and executes as it does alone. The End waits once for the group launches it queued.
 * The first error of the execution is returned and later recorded calls are not run; the group is cleared either
 * way. nexrRingCommGetQueued reports 5 after an End that queued at least one group launch.
 *
 * nexrRingGroupGetStats — since creation or the last reset: calls recorded, group launches, fill launches (tables
 * beyond the kernel arguments), calls run singly, and cuts (conflicts between works that closed the open
 * launches of a nexrFlatGroup call). reset != 0 zeroes the counters after reading them.
 */
typedef struct {
  uint64_t calls, groupLaunches, fillLaunches, singles, cuts;
} nexrRingGroupStats;
NEXR_API nexrResult_t nexrRingGroupStart(nexrRingComm_t comm);
NEXR_API nexrResult_t nexrRingGroupEnd(nexrRingComm_t comm);
NEXR_API nexrResult_t nexrRingGroupGetStats(nexrRingComm_t comm, nexrRingGroupStats* stats, int reset);

/* User-created reduction ops: ncclRedOpCreatePreMulSum / ncclRedOpDestroy (reference src/nccl.h.in:305-325,
 * src/enqueue.cc:2447-2518) and the `default:` row of hostToDevRedOp (:2266-2275). Under the op every rank's own
 * input is multiplied by that rank's own scalar (rounded to the datatype) before the sum; nothing else is scaled.
 *
 * A thread-rank communicator holds all n ranks, so scalars[r] is rank r's scalar (the reference's ranks each call
 * create with their own). nexrScalarHostImmediate: scalars[r] points to one element of `datatype` in host memory,
 * copied at creation. nexrScalarDevice: scalars[r] is kept and dereferenced during every collective that uses the
 * op (element-aligned; any memory the HIP runtime knows, device memory included; on a communicator that never
 * touches HIP, because every step is a caller's function, the host's own memory). A device-resident scalar is
 * read once per call and rank at the start of the call, by a copy ordered behind the rank's stream; the calls
 * are blocking, so that is while the collective runs, and the next call sees a value rewritten in between.
 *
 * *op is nexrNumOps + ix. The table is the reference's (:2453-2471, :2508-2515): its capacity doubles from 4 and
 * the free list is last-in first-out, so a destroyed handle is the next one handed out. Destroying an op does not
 * wait for anything: the calls are blocking, so no collective is using it.
 *
 * nexrInvalidArgument, before any device call: destroying a built-in op; a handle that is out of range, already
 * destroyed or never issued, in destroy or in a collective (:2491-2512, argcheck.cc:66); a collective whose
 * datatype is not the op's (:2269-2273); fp8 or an unknown datatype or residence; a null `scalars` or a null
 * entry. nexrInvalidUsage from create on a process-rank communicator (not built; its collectives therefore know
 * no handle).
 *
 * Which entries take a handle wherever they take a built-in op: nexrRingAllReduce, nexrRingReduceScatter,
 * nexrRingReduce, nexrTreeAllReduce, their ...Flat forms, and the one-rank path of each. Which keep refusing one
 * with nexrInvalidArgument, exactly as they refuse op 5 without this: the symmetric entries (Sum only), the
 * nexrPeerRing* entries, and the extras library's resident and send/recv entries (include/nexr_extras.h).
 *
 * How a call with a user op runs. Every rank's Primitives carries its own rank's scalar, which is all the
 * host-sequenced SIMPLE / LL / LL128 steps (host or device memory), the queued LL launches and the per-rank LL
 * runs on the device need: their pre-op applies to the rank's own input only. The launches that carry ONE
 * redOpArg for all ranks (the group launches of nexrRingCommSetLLGroup / nexrRingCommSetSimpleGroup and the flat
 * launches) serve a user op when all n scalars are bit-equal once read, and the call then runs exactly as
 * ncclAvg's PreMulSum does. With differing scalars:
 *   - a group option falls back to the mode the call would have run without it, one more case of the fall-back
 *     lists of nexrRingCommSetLLGroup and nexrRingCommSetSimpleGroup; nexrRingCommGetQueued reports what ran;
 *   - on a device-memory communicator the ...Flat entries, and the plain calls under nexrRingCommSetFlat, run
 *     the launches with a scalar per rank (nexrFlatAllReducePreMul, nexrFlatReduceScatterPreMul,
 *     nexrFlatReducePreMul, nexrFlatTreeAllReducePreMul, include/nexr.h): one launch, the same bytes, 4 reported;
 *   - a host-memory communicator has no such launch: under nexrRingCommSetFlat the call runs host-sequenced, as
 *     without the option, and reports 0; its explicit ...Flat entries return nexrInvalidUsage.
 * A device-resident scalar on those device-memory flat calls is not read by the host at all: the kernel reads it
 * (also when all n turn out equal), so what the communicator's first stream, or anything ordered before the
 * call, wrote last is what counts. */
typedef enum { nexrScalarDevice = 0, nexrScalarHostImmediate = 1 } nexrScalarResidence_t; /* = ncclScalarResidence_t */
NEXR_API nexrResult_t nexrRingRedOpCreatePreMulSum(nexrRingComm_t comm, int* op, const void* const* scalars,
                                                   int datatype, int residence);
NEXR_API nexrResult_t nexrRingRedOpDestroy(nexrRingComm_t comm, int op);

/* The tree links of `rank` in this communicator's topology: *up (-1 at the root) and down[0..2]
 * (-1 when absent, children packed first as setTreeDown does). */
NEXR_API nexrResult_t nexrTreeTopology(nexrRingComm_t comm, int rank, int* up, int* down);

/* How this communicator's rank threads wait for each device step before posting it (*word = 1: a
 * hipStreamWriteValue32 completion word the thread spins on; 0: hipStreamSynchronize). The word is
 * the default only when every rank runs on the same GPU; when the ranks span GPUs (thread ranks on
 * several devices, or process ranks whose published GPUs differ) the default is the
 * synchronisation. NEXR_STEP_WAIT=word / sync, read once per process, forces either. */
NEXR_API nexrResult_t nexrRingCommGetStepWait(nexrRingComm_t comm, int* word);

/* How the last thread-rank ring collective on this communicator ran its LL steps (and, while the group
 * option below is on, the last nexrTreeAllReduce: 3 as group launches, 0 when it fell back to host
 * sequencing; with the option off a tree call leaves the report untouched). *queued = 2: runs
 * on the device (nexrReduceCopyLLSteps), up to 96 steps per launch, the peers' data found by the
 * kernel's flag poll (prims_ll.h:38-93) and the slot credits by its poll of the receivers' head words in
 * device memory (waitSend / postRecv, :55-83), no host wait until the collective's end (the default
 * where 1 is possible and the communicator uses the library's own LL kernels; NEXR_LL_RUN=0 falls back
 * to 1). 1: queued, each step's kernel on the rank's stream with no host wait after it, the slots a
 * step read released once a completion ticket behind it lands (one per NEXR_LL_TICKET_EVERY steps,
 * default 4). 0: host-sequenced (SIMPLE and LL128 without their group options, ranks on several GPUs, host
 * memory, NEXR_LL_ASYNC=0, or more rank streams on a GPU than it has hardware queues beside the default
 * stream's). 3: group launches on one stream (nexrRingCommSetLLGroup, below; LL and LL128;
 * nexrRingCommSetSimpleGroup for SIMPLE). 4: one flat launch (nexrRingCommSetFlat, above). */
NEXR_API nexrResult_t nexrRingCommGetQueued(nexrRingComm_t comm, int* queued);

/* Opt-in: run the LL steps of every rank (and channel) of a ring collective in group launches on ONE
 * stream (nexrReduceCopyLLStepsGroup, include/nexr.h). With on != 0, the five ring collectives record
 * each (channel, rank)'s whole step list on the rank threads, the calling thread then queues the group
 * launches on one stream of the communicator, waits once and publishes the host counters, and
 * nexrRingCommGetQueued reports 3. No rank stream needs a hardware queue of its own, so the cap of mode
 * 1 / 2 (GPU_MAX_HW_QUEUES - 1 rank streams on a GPU) does not apply: 4-8 ranks, or several channels,
 * run on the device too. The communicator owns the launches' workspace. The flag rule, the cleanup
 * counter and the status word (a timeout, or 2 for a relayed abort) work as in mode 2, and the option may
 * be switched between collectives in either direction: every launch of either mode re-stores the device
 * head words from the step counters both modes keep. A collective falls back to the mode it would have
 * run without the option when its ranks span several GPUs, the communicator has a caller's llFn, the
 * collective has more than NEXR_LL_GROUP_MAX_MEMBERS (channel, rank) members, or the group's grid is not
 * resident at once on the GPU.
 *
 * nexrTreeAllReduce takes the option too. Every Primitives of the call is a member: the root with its
 * receive and send connections to every child, and every other rank's reduce-up and broadcast-down halves,
 * 2n - 1 members per channel (up to 3 + 3 connections each). The rank threads record, the calling thread
 * queues the group launches, and the call reports 3. It runs host-sequenced instead, as without the option
 * and from the step counters as they were, and reports 0, when the ranks span several GPUs, the
 * communicator has a caller's llFn / ll128Fn or waits by hipStreamSynchronize, the call has more than
 * NEXR_LL_GROUP_MAX_MEMBERS members over its channels, or the grid is not resident at once. Under LL a
 * member with several send connections cleans every one of them on its cleaning steps. Ring and tree calls
 * may be mixed and the option toggled between them: they use disjoint connections.
 *
 * LL128 communicators take the option too: their step lists go to nexrReduceCopyLL128StepsGroup, whose
 * hand-off is ordered by construction (include/nexr.h), the only way LL128 steps of two ranks run at the
 * same time; with the option off (the default) an LL128 communicator stays host-sequenced, mode 0, and
 * every fall-back above (a caller's ll128Fn in place of llFn) returns to that. There is no flag rule and
 * no cleanup for LL128.
 *
 * nexrInvalidUsage unless the communicator has thread ranks, the LL or LL128 protocol and device memory. */
NEXR_API nexrResult_t nexrRingCommSetLLGroup(nexrRingComm_t comm, int on);

/* SIMPLE step lists in group launches (nexrReduceCopySimpleStepsGroup, include/nexr.h): nexrRingCommSetLLGroup
 * for the SIMPLE protocol, whose steps otherwise cost one launch, one completion wait and the host's
 * head / tail stores each. With on != 0 the five ring collectives record each (channel, rank)'s slices on
 * the rank threads (Prims::genericOp makes no waits and no launches; zero-size slices are recorded too),
 * the calling thread queues the group launches on one stream, waits once and publishes the host head /
 * tail, and nexrRingCommGetQueued reports 3. The first switch-on allocates and zeroes a tail block and a
 * head block of NEXR_SIMPLE_CREDIT_BYTES per ring connection; communicators that never switch it on are
 * unchanged. The grid starts at the call's default (a workgroup per 4 KiB tile of a slice, 256 at most per
 * member) and is halved down to one workgroup per member while the call answers that it is not resident at
 * once. A collective is host-sequenced as without the option, from the counters as they were, and reports
 * 0, when its ranks span several GPUs, the communicator has a caller's fn or waits for its steps by
 * hipStreamSynchronize, the collective has more than NEXR_LL_GROUP_MAX_MEMBERS (channel, rank) members, or
 * the grid is not resident even at one workgroup per member. The option may be toggled between collectives,
 * and collectives with 1-step slices (Reduce, Broadcast) and 2-step slices may alternate: every launch
 * re-stores its head and tail words from the step counters both modes keep. nexrTreeAllReduce does not
 * take it. Opt-in, and not always a gain: a 4 MiB fp32 all-reduce on one MI355X took 0.181-0.210 ms with
 * the option against 0.167-0.197 ms host-sequenced at 2 ranks (SLOWER), 0.375-0.407 against 0.384-0.425 at
 * 4 ranks, 0.831-0.850 against 1.047-1.076 at 8 ranks and 0.501-0.524 against 0.570-0.601 at 4 ranks x 2
 * channels (profiles/r10a_simple_group_probe.json).
 *
 * nexrInvalidUsage unless the communicator has thread ranks, the SIMPLE protocol and device memory. */
NEXR_API nexrResult_t nexrRingCommSetSimpleGroup(nexrRingComm_t comm, int on);

/* DirectWrite for the SIMPLE ring collectives (reference src/device/prims_simple.h:148-164, :258-269). With
 * on != 0 the caller states that the user buffers it will pass are registered (the reference's regUsed): a
 * sender then writes each slice into the NEXT rank's recvbuff at the slice's output offset instead of a FIFO
 * slot, the receiver reads it from its own recvbuff, a copy whose source is its destination is skipped, and
 * the last step of every chunk (directRecv) moves no data: it only waits and posts. Thread ranks know every
 * buffer when the call starts, so nothing is exchanged. Host or device memory both qualify. A collective runs
 * direct where the reference registers (src/register/coll_reg.cc:177-178): AllGather and Broadcast always,
 * in place or not; AllReduce only when every rank is out of place (its reduce-scatter half uses the
 * recvbuffs as scratch); ReduceScatter and Reduce never. Device-memory ranks on several GPUs fall back to
 * FIFOs too, and nexrTreeAllReduce ignores the option. A call that is not eligible runs exactly as without
 * the option; the results are bit-identical either way. Direct and FIFO slices share the step counters, so
 * the option may be toggled between collectives, and it combines with nexrRingCommSetSimpleGroup (the
 * records then carry the direct bits and the group call is nexrReduceCopySimpleStepsGroupDirect,
 * include/nexr.h). Host-sequenced, a skipped copy is one fn call with one source and the send destinations,
 * and a directRecv slice makes no fn call. Derived: 5n - 4 against 6n - 4 memory accesses per chunk element
 * of an n-rank all-reduce, 2n - 1 against 3n - 1 for an out-of-place all-gather. Measured on one MI355X, 4 MiB
 * of fp32 per rank, medians of 30 calls, two runs each (profiles/r11a_simple_direct_probe.json, DESIGN §8.3;
 * a setting's two runs differ by up to 15-25 %): host-sequenced, direct against FIFOs, all-reduce at 2 / 4 / 8
 * ranks 0.13-0.16 / 0.34-0.37 / 1.02-1.03 ms against 0.15-0.18 / 0.38-0.40 / 1.06-1.08, all-gather at 2 / 8
 * ranks 0.12-0.13 / 0.63-0.66 against 0.14-0.15 / 0.67-0.68, broadcast 0.15-0.17 / 0.39 against 0.19 /
 * 0.38-0.40; in group launches direct is level with FIFOs within that spread and SLOWER for the broadcast at
 * 2 ranks (0.15-0.16 against 0.13-0.14) and the all-reduce at 4 and 8 ranks (0.36-0.38 against 0.35, 0.83-0.88
 * against 0.77-0.85). Opt-in.
 *
 * nexrInvalidUsage unless the communicator has thread ranks and the SIMPLE protocol. */
NEXR_API nexrResult_t nexrRingCommSetDirect(nexrRingComm_t comm, int on);

/* The last thread-rank ring collective's send slices of either kind over all ranks and channels (zero-size
 * slices included): *directSlices went into a peer's recvbuff, *fifoSlices into a FIFO slot. */
NEXR_API nexrResult_t nexrRingCommGetDirect(nexrRingComm_t comm, uint64_t* directSlices, uint64_t* fifoSlices);

/* The LL flag rule of this communicator (nexrLLFlagRule, include/nexr.h; NULL or {0, 0x7ffffff8}: the
 * production rule, the default; {0x100, 0x78}: the reference's TEST_LL_CLEANUP), for every channel. Its LL
 * steps take their flags from it, and on a cleaning send step rewrite the rest of the step's slot as
 * {0, flag, 0, flag} (reference incSend, src/device/prims_ll.h:85-93) in every mode: host-sequenced and
 * queued steps after the step's llFn and before its tail is published (nexrLLCleanSlot on the rank's
 * stream for device-memory FIFOs, CPU stores for host-memory ones), runs on the device inside the
 * launch (nexrReduceCopyLLStepsRule). LL128 is not affected (64-bit flags; the reference does no
 * cleanup there). Only before the communicator's first collective: nexrInvalidUsage afterwards; an
 * invalid rule (for the FIFO's 8 slots) returns nexrInvalidArgument. */
NEXR_API nexrResult_t nexrRingCommSetLLFlagRule(nexrRingComm_t comm, const nexrLLFlagRule* rule);

/* Diagnostics of that cleanup. *minSendStep: the smallest send-step counter among the connections that
 * have sent (0 when none has); *cleanedSteps: cleaning send steps since creation, over all connections
 * and channels (one per connection and step). */
NEXR_API nexrResult_t nexrRingCommGetLLCleanup(nexrRingComm_t comm, uint64_t* minSendStep, uint64_t* cleanedSteps);

NEXR_API nexrResult_t nexrRingCommDestroy(nexrRingComm_t comm);

/*
 * Process ranks over peer memory (the §8(f) xGMI ring step): one process per GPU, each process one
 * rank of the same ring schedule. Like the reference's P2P transport in write mode
 * (src/transport/p2p.cc:231-240, :299, :402, :514-515, :542-543): every rank allocates the FIFO it
 * receives into, exports it with hipIpcGetMemHandle, and maps the next rank's FIFO with
 * hipIpcOpenMemHandle; its reduce-copy kernels write straight into that peer FIFO (over xGMI when
 * the ranks drive different GPUs). Step counters and the rendezvous live in a POSIX shared-memory
 * segment `shmName` (single node): every rank passes the same fresh name ("/name", no other '/');
 * the last rank to destroy its communicator unlinks it. Create blocks until all nRanks joined
 * (bounded by timeoutMs). Every rank must then issue the same sequence of nexrPeerRingAllReduce
 * calls (same count, datatype, op). Buffers are device memory on `device`. Destroy with
 * nexrRingCommDestroy.
 */
typedef struct {
  int nRanks;
  int rank;
  int device;          /* HIP device of this rank's buffers and kernels */
  size_t buffBytes;    /* 0 = the protocol default (as nexrRingConfig) */
  int protocol;        /* nexrRingProto_t */
  int timeoutMs;       /* rendezvous and per-wait bound; 0 = 60000 */
  const char* shmName; /* shared by all ranks of this communicator */
} nexrPeerRingConfig;

NEXR_API nexrResult_t nexrPeerRingCommCreate(nexrRingComm_t* comm, const nexrPeerRingConfig* config);

/* ncclAllReduce for this process's rank (sendbuff/recvbuff on config->device; in-place allowed). */
NEXR_API nexrResult_t nexrPeerRingAllReduce(nexrRingComm_t comm, const void* sendbuff, void* recvbuff, size_t count,
                                            int datatype, int op);

/* The other ring collectives for this process's rank, arguments as in the thread-rank versions. */
NEXR_API nexrResult_t nexrPeerRingReduceScatter(nexrRingComm_t comm, const void* sendbuff, void* recvbuff,
                                                size_t recvcount, int datatype, int op);
NEXR_API nexrResult_t nexrPeerRingAllGather(nexrRingComm_t comm, const void* sendbuff, void* recvbuff,
                                            size_t sendcount, int datatype);
NEXR_API nexrResult_t nexrPeerRingReduce(nexrRingComm_t comm, const void* sendbuff, void* recvbuff, size_t count,
                                         int datatype, int op, int root);
NEXR_API nexrResult_t nexrPeerRingBroadcast(nexrRingComm_t comm, const void* sendbuff, void* recvbuff, size_t count,
                                            int datatype, int root);

#ifdef __cplusplus
}
#endif

#endif /* NEXR_RING_H_ */
