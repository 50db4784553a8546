// nexr_internal.h — shared between the C-ABI host code (nexr_api.cpp) and the per-datatype
// kernel objects (nexr_kernels.hip). Not installed; not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/nexr.h"

namespace nexr {

constexpr int kBlock = 256;  // 4 waves of 64 lanes per workgroup

// Launch parameters of one reduce-copy, passed by value as the kernel argument.
//
// Element range layout (host computes it, see planLayout in nexr_api.cpp):
//   [0, head)                    edge elements before dst[0]'s next 128-B boundary (scalar path)
//   [head, head + nPacks*EPP)    the packed body: pack i = 16 contiguous bytes of every buffer
//   [.., nElts)                  tail edge elements (scalar path)
// When the pointers share a 16-B phase every body access is 16-B aligned; otherwise (`unaligned`)
// the others are unaligned 16-B accesses.
struct RCParams {
  const char* src[NEXR_MAX_SRCS];
  char* dst[NEXR_MAX_DSTS];
  uint64_t pre[NEXR_MAX_SRCS];  // raw pre-op scalar bits per src (PreMulSum), reduce_kernel.h:145,:166
  const void* prePtr;           // if non-null, pre[0] is loaded from this device address (onerank.cc:32-42)
  uint64_t redArg;              // op argument (MinMax bit 0, SumPostDiv divisor<<1|signed)
  uint64_t nElts;
  uint64_t head;                // edge elements before the body
  uint64_t nPacks;              // 16-B packs in the body
  int nDsts;
  int nPreOp;                   // pre-op applies to srcs[s] for s < nPreOp
  int postOp;
  int unaligned;  // no common 16-B phase: body packs use unaligned 16-B accesses (diagnostics)
};

// Launch parameters of one LL-protocol step (nexr_ll.hip; reference src/device/prims_ll.h:218-283).
struct LLParams {
  const char* src;                  // user buffer (nullable)
  const char* recv[NEXR_MAX_SRCS];  // peer LL lines of this step
  uint32_t recvFlag[NEXR_MAX_SRCS];
  char* dst;                        // user buffer (nullable)
  char* send[NEXR_MAX_DSTS];
  uint32_t sendFlag[NEXR_MAX_DSTS];
  uint64_t nElts;
  uint64_t redArg;
  uint32_t* status;                 // set to 1 when a recv flag never arrived (nullable)
  uint64_t timeoutTicks;            // s_memrealtime ticks (100 MHz) before giving up
  int nRecv, nSend, srcIsInput, postOp;
  int firstWins;                    // nexrSemanticsShipped: every reduce returns its first operand
};
hipError_t launch_ll(int dt, const LLParams& a, int op, int grid, hipStream_t s);

// A run of LL steps of one Primitives in one launch (nexrReduceCopyLLSteps; nexr_ll.hip). Workgroup w
// owns line tiles t = w, w + grid, ... of every step and its wave v the same lines of each tile, on both
// ends of a connection, so the credit of a slot is per wave: head word (w, v) of a connection holds the
// steps the receiver's wave v of workgroup w has read.
constexpr int kLLStepsMax = 96;        // steps per launch: the parameter block stays under 4 KiB
constexpr int kLLHeadStride = 16;      // bytes between a connection's head words (one per wave)
constexpr int kLLStepsMaxGrid = NEXR_LL_HEAD_BYTES / (kLLHeadStride * (kBlock / 64));
struct LLStepsParams {
  const char* input;
  char* output;
  const char* recvFifo[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t* recvHead[NEXR_LL_STEPS_MAX_PEERS];
  char* sendFifo[NEXR_LL_STEPS_MAX_PEERS];
  const uint64_t* sendHead[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t recvStep[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t sendStep[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t slotBytes;
  uint64_t redArg;
  uint32_t* status;
  uint64_t timeoutTicks;
  int nRecv, nSend, nSlots, nSteps;
  int firstWins;
  // The flag rule (nexrLLFlagRule): NCCL_LL_FLAG(a) = (uint32_t)a & flagMask (flagMax - 1, or all ones).
  // A send step s also cleans its slot when (s & cleanMask) == cleanMask: the host ends the launch at such
  // a step; bit j of cleanLast says that send connection j cleans at the launch's last step, whose send
  // counter on that connection is cleanStep[j].
  uint32_t flagMask, cleanLast;
  uint64_t cleanStep[NEXR_LL_STEPS_MAX_PEERS];
#ifdef NEXR_LL_STEPS_TRACE
  uint64_t* trace;  // tuning harness only (tools/ll_steps_trace.hip)
#endif
  nexrLLStep step[kLLStepsMax];
};
static_assert(sizeof(LLStepsParams) <= 4096, "kernel argument block");
hipError_t launch_ll_steps(int dt, const LLStepsParams& a, int op, int grid, hipStream_t s);

// The runs of nMembers Primitives in one launch (nexrReduceCopyLLStepsGroup): `table` is nMembers
// parameter blocks in device memory (kLLGroupEntryBytes apart), the grid nMembers * G workgroups.
constexpr size_t kLLGroupEntryBytes = sizeof(LLStepsParams);
static_assert(kLLGroupEntryBytes % 8 == 0, "table entries stay 8-byte aligned");
hipError_t launch_ll_group(int dt, int op, const LLStepsParams* table, int nMembers, int G, hipStream_t s);
hipError_t ll_group_blocks_per_cu(int dt, int op, int* blocks);

// The flag-wrap cleanup of one step for callers of the single-step kernel (nexrLLCleanSlot): lines
// [firstLine, slotLines) of every slot become {0, flag, 0, flag} (reference incSend, prims_ll.h:85-93).
struct LLCleanParams {
  char* send[NEXR_MAX_DSTS];
  uint32_t flag[NEXR_MAX_DSTS];
  uint64_t firstLine, slotLines;
  int nSend;
};
hipError_t launch_ll_clean(const LLCleanParams& a, int grid, hipStream_t s);

// Launch parameters of one LL128-protocol step (nexr_ll.hip; reference src/device/prims_ll128.h).
// Wire: 2 KiB slices of 16 x 128-B lines carrying 1920 data bytes; word 15 of every line is the flag.
constexpr int kLL128SliceBytes = 2048;
constexpr int kLL128SliceData = 1920;
// Work per workgroup iteration (nexr_ll.hip): LL, kLLU sub-tiles of 2 * kBlock lines (8 data bytes
// each); LL128, kLL128U sub-tiles of kBlock 16-byte wire units. One sub-tile (4 KiB of data or wire
// per workgroup) is fastest at the protocols' step sizes, 32 KiB-4 MiB, by up to 1.8x over four, and
// for LL at 64 MiB as well; four gain <= 10 % only for LL128 at 64 MiB (tools/ll_bits.hip,
// profiles/r02s5_ll_bits.txt).
#ifndef NEXR_LL_U  // overridable only by tuning harnesses (tools/ll_bits.hip)
#define NEXR_LL_U 1
#endif
constexpr int kLLU = NEXR_LL_U;
constexpr int kLLSubLines = 2 * kBlock;
constexpr int kLLTileLines = kLLU * kLLSubLines;
constexpr int kLL128U = NEXR_LL_U;
constexpr int kLL128TileUnits = kLL128U * kBlock;
struct LL128Params {
  const char* src;
  const char* recv[NEXR_MAX_SRCS];
  uint64_t recvFlag[NEXR_MAX_SRCS];
  char* dst;
  char* send[NEXR_MAX_DSTS];
  uint64_t sendFlag[NEXR_MAX_DSTS];
  uint64_t nElts;
  uint64_t redArg;
  uint32_t* status;
  uint64_t timeoutTicks;
  int nRecv, nSend, srcIsInput, postOp;
  int firstWins;  // as LLParams
};
hipError_t launch_ll128(int dt, const LL128Params& a, int op, int grid, hipStream_t s);

// LL128 step lists of nMembers Primitives in one launch (nexrReduceCopyLL128StepsGroup; nexr_ll.hip). The
// table entry is the LL group's LLStepsParams (flagMask, cleanLast and cleanStep unused: 64-bit flags, no
// cleanup), so nexrLLGroupWorkspaceBytes sizes both calls' workspaces. Tile t (kLL128TileUnits wire units)
// of a step belongs to workgroup t % G, G from slotBytes alone, at most kLLStepsMaxGrid.
hipError_t launch_ll128_group(int dt, int op, const LLStepsParams* table, int nMembers, int G, hipStream_t s);
hipError_t ll128_group_blocks_per_cu(int dt, int op, int* blocks);

// SIMPLE step lists of nMembers Primitives in one launch (nexrReduceCopySimpleStepsGroup; nexr_simple.hip).
// A record is one slice of genericOp; tile t (kSimpleTileBytes from the slice's start) belongs to workgroup
// t % G on both ends of a connection, and the credit is per workgroup: word w (kSimpleCreditStride apart)
// of a connection's tail block says how far the sender's workgroup w has published, word w of its head
// block how far the receiver's workgroup w has released.
constexpr int kSimpleTileBytes = 4096;
constexpr int kSimpleCreditStride = 16;
constexpr int kSimpleMaxGrid = NEXR_SIMPLE_CREDIT_BYTES / kSimpleCreditStride;
static_assert(kSimpleMaxGrid == NEXR_SIMPLE_GROUP_MAX_GRID, "public grid limit must match the credit block");
struct SimpleStepsParams {
  const char* input;
  char* output;
  const char* recvFifo[NEXR_LL_STEPS_MAX_PEERS];
  const uint64_t* recvTail[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t* recvHead[NEXR_LL_STEPS_MAX_PEERS];
  char* sendFifo[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t* sendTail[NEXR_LL_STEPS_MAX_PEERS];
  const uint64_t* sendHead[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t recvStep[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t sendStep[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t slotBytes;
  uint64_t redArg;
  uint32_t* status;
  uint64_t timeoutTicks;
  int nRecv, nSend, nSlots, nSteps;
  int firstWins;     // nexrSemanticsShipped: every reduce returns source 0
  int stepPerSlice;  // counter steps (and slots) per record
  nexrLLStep step[kLLStepsMax];
};
static_assert(sizeof(SimpleStepsParams) % 8 == 0, "table entries stay 8-byte aligned");
hipError_t launch_simple_group(int dt, int op, const SimpleStepsParams* table, int nMembers, int G, hipStream_t s);
hipError_t simple_group_blocks_per_cu(int dt, int op, int* blocks);

// The same with DirectWrite connections (nexrReduceCopySimpleStepsGroupDirect): a kernel variant of its own
// (the FIFO-only kernels stay as they are) and a table entry that adds, per member, the peers' output
// buffers of its direct send connections and whether its receive connection is direct.
struct SimpleDirectParams : SimpleStepsParams {
  char* sendDirect[NEXR_LL_STEPS_MAX_PEERS];  // nullptr: the connection uses its FIFO
  int recvDirect;                             // receive connection 0 is direct (then nRecv == 1)
  int pad;
};
static_assert(sizeof(SimpleDirectParams) % 8 == 0, "table entries stay 8-byte aligned");
hipError_t launch_simple_group_direct(int dt, int op, const SimpleDirectParams* table, int nMembers, int G,
                                      hipStream_t s);
hipError_t simple_group_direct_blocks_per_cu(int dt, int op, int* blocks);

// The symmetric all-reduce in one launch (nexrSymAllReduce; nexr_sym.hip): the 2n pointers and the ownership
// plan the host derives from rank 0's pointers (symPlan, nexr_api.cpp; reference
// src/device/symmetric/all_reduce.hh:199-252). Offsets are bytes from every buffer's start.
struct SymParams {
  const char* in[NEXR_SYM_MAX_RANKS];
  char* out[NEXR_SYM_MAX_RANKS];
  uint64_t p1Off, p1Pieces;  // pass 1: 2048-byte pieces from p1Off, piece i owned by rank i % n
  uint64_t p2Off, p2Pieces;  // pass 2: 512-byte pieces from p2Off, piece i owned by rank i % n
  uint64_t preElts, sufOff;  // ends: element e < preElts at e, the others from byte sufOff on;
  uint64_t nEnds;            //   nEnds elements in all, element e owned by rank (e / 32) % n
  int nRanks;
  int nFold;  // inputs that enter the fold from the owner's on: nRanks, or 1 under nexrSemanticsShipped
};
static_assert(sizeof(SymParams) <= 4096, "kernel argument block");
hipError_t launch_sym_all_reduce(int dt, const SymParams& p, unsigned grid, hipStream_t s);

// The symmetric reduce-scatter and all-gather in one launch (nexrSymReduceScatter, nexrSymAllGather;
// nexr_sym.hip). Chunk r of an input (reduce-scatter) or of an output (all-gather) starts at byte
// r * chunkBytes / r * nBytes; the kernels cut every chunk from its byte 0 themselves.
struct SymRsParams {
  const char* in[NEXR_SYM_MAX_RANKS];  // nRanks * chunkBytes bytes each
  char* out[NEXR_SYM_MAX_RANKS];       // chunkBytes bytes each
  uint64_t chunkBytes;                 // nElts * esz
  int nRanks;
  int nFold;  // inputs that enter the fold from rank r's on: nRanks, or 1 under nexrSemanticsShipped
};
struct SymAgParams {
  const char* in[NEXR_SYM_MAX_RANKS];  // nBytes bytes each
  char* out[NEXR_SYM_MAX_RANKS];       // nRanks * nBytes bytes each
  uint64_t nBytes;
  uint64_t inPlace;  // bit r: inputs[r] == outputs[r] + r * nBytes, rank r's own output is not stored
  int nRanks;
};
static_assert(NEXR_SYM_MAX_RANKS <= 64, "SymAgParams::inPlace is one bit per rank");
static_assert(sizeof(SymRsParams) <= 4096 && sizeof(SymAgParams) <= 4096, "kernel argument block");
hipError_t launch_sym_reduce_scatter(int dt, const SymRsParams& p, unsigned grid, hipStream_t s);
hipError_t launch_sym_all_gather(const SymAgParams& p, unsigned grid, hipStream_t s);

// The symmetric LL collectives in one launch (nexrSymLLAllReduce, nexrSymLLReduceScatter, nexrSymLLAllGather;
// nexr_sym.hip): a grid of nRanks * nBlocks teams, rank fastest. coll: 0 all-reduce, 1 reduce-scatter, 2
// all-gather. nBytes is what a team splits into 8-byte packs: the all-reduce's buffer, the reduce-scatter's
// chunk (= output), the all-gather's input; below 2^31.
struct SymLLParams {
  const char* in[NEXR_SYM_MAX_RANKS];
  char* out[NEXR_SYM_MAX_RANKS];
  char* win[NEXR_SYM_MAX_RANKS];  // the windows: header, then per block two buffers of nRanks * round lines
  uint64_t nBytes;
  uint32_t* status;
  uint64_t timeoutTicks;
  int nRanks, nBlocks;
  int firstWins;  // nexrSemanticsShipped: every add returns its first operand
};
static_assert(sizeof(SymLLParams) <= 4096, "kernel argument block");
hipError_t launch_sym_ll(int coll, int dt, const SymLLParams& p, hipStream_t s);
hipError_t sym_ll_blocks_per_cu(int coll, int dt, int* blocks);

// The ring all-reduce, reduce-scatter and reduce in one launch with the ring's bytes (nexrFlatAllReduce,
// nexrFlatReduceScatter, nexrFlatReduce; nexr_flat.hip). A region is what a wave's pieces are cut from: the
// all-reduce's and the reduce's whole buffer, one chunk of the reduce-scatter (chunk d of an input starts at
// byte d * regionBytes). The all-reduce's channel parts ride in the kernel arguments, or, beyond
// kFlatInlineParts of them, in a stream-ordered workspace (`ext`). A launch covers the byte window
// [winBeg, winEnd) of every region (winBeg a multiple of the 2048-byte piece; 0 and regionBytes: the whole
// region). Positions stay global: a pointer addresses `ptr + region offset` whatever the window, so a buffer
// that holds only the window's bytes is passed biased by -winBeg (the host entries' staged windows).
enum { kFlatAllReduce = 0, kFlatReduceScatter = 1, kFlatReduce = 2 };
constexpr int kFlatInlineParts = NEXR_FLAT_INLINE_PARTS;
struct FlatParams {
  static constexpr bool kPerRank = false;  // one pre-op factor for the call: redArg
  static constexpr bool kOneItem = false;  // a launch of its own: the grid strides over every item
  const char* in[NEXR_SYM_MAX_RANKS];
  char* out[NEXR_SYM_MAX_RANKS];  // the reduce: out[root] only
  uint64_t regionBytes;
  uint64_t redArg;
  uint64_t winBeg, winEnd;  // the bytes of every region that this launch covers
  const nexrFlatPart* ext;  // non-null: the parts are there, not in parts[]
  int coll, nRanks;
  int nFold;      // inputs that enter the chain: nRanks, or 1 under nexrSemanticsShipped
  int shift;      // the folded inputs start at rank s + shift (0, or the chain's last rank under shipped SIMPLE)
  int userFirst;  // SIMPLE: the rank's own input is a step's first operand; else the partial is
  int preOp, postOp, root, nParts;
  int nOut;  // the all-reduce stores out[0 .. nOut): nRanks, or fewer where outputs share a buffer
  nexrFlatPart parts[kFlatInlineParts];
};
static_assert(sizeof(FlatParams) <= 4000, "kernel argument block");
// nexrFlatAllReducePreMul / nexrFlatReduceScatterPreMul / nexrFlatReducePreMul: FlatParams' fields by the same
// names (the kernel code is one template over both), PreMulSum implied, and rank r's pre-op scalar in scalars[r]:
// the raw bits of one element, or with scalarsArePtrs the device address the kernel reads it from. The n scalars
// take the room of inline parts: kFlatPreMulInlineParts of them ride in the arguments, longer lists in `ext`.
constexpr int kFlatPreMulInlineParts = NEXR_FLAT_PREMUL_INLINE_PARTS;
struct FlatPreMulParams {
  static constexpr bool kPerRank = true;
  static constexpr bool kOneItem = false;
  const char* in[NEXR_SYM_MAX_RANKS];
  char* out[NEXR_SYM_MAX_RANKS];
  uint64_t scalars[NEXR_SYM_MAX_RANKS];
  uint64_t regionBytes;
  uint64_t winBeg, winEnd;
  const nexrFlatPart* ext;
  int coll, nRanks;
  int nFold, shift, userFirst;
  int preOp, postOp, root, nParts;
  int nOut;
  int scalarsArePtrs, pad;
  nexrFlatPart parts[kFlatPreMulInlineParts];
};
static_assert(sizeof(FlatPreMulParams) <= 4000, "kernel argument block");
hipError_t launch_flat_premul(int dt, const FlatPreMulParams& p, unsigned grid, hipStream_t s);
struct FlatPartsFill {
  nexrFlatPart* dst;
  int n, pad;
  nexrFlatPart parts[kFlatInlineParts];
};
hipError_t launch_flat(int dt, int op, const FlatParams& p, unsigned grid, hipStream_t s);
hipError_t launch_flat_parts(const FlatPartsFill& f, hipStream_t s);

// The tree all-reduce and the broadcast in one launch (nexrFlatTreeAllReduce, nexrFlatBroadcast;
// nexr_flat_tree.hip). A tree travels as a program of one-byte instructions, opcode << 6 | rank, and as the
// ranks in the order the program consumes their inputs (what the kernel's loads run ahead on).
enum { kFlatTreeLeaf = 0, kFlatTreeJoin = 1, kFlatTreePush = 2, kFlatTreeMerge = 3 };
constexpr int kFlatTreeSlots = NEXR_FLAT_TREE_SLOTS;  // live values: the accumulator and the saved ones
constexpr int kFlatTreeInlineParts = NEXR_FLAT_TREE_INLINE_PARTS;
constexpr int kFlatTreeProgBytes = 3 * NEXR_SYM_MAX_RANKS;  // 3n - 2 instructions at the most
struct FlatTreeProgram {
  uint32_t code[kFlatTreeProgBytes / 4];    // bytes, packed little-endian: the kernel loads dwords
  uint32_t order[NEXR_SYM_MAX_RANKS / 4];   // rank of the j-th LEAF / JOIN, packed likewise
  int nCode, nIn;                           // nIn: n, or 1 under nexrSemanticsShipped
};
struct FlatTreeParams {
  static constexpr bool kPerRank = false;  // one pre-op factor for the call: redArg
  const char* in[NEXR_SYM_MAX_RANKS];
  char* out[NEXR_SYM_MAX_RANKS];
  uint64_t nBytes;
  uint64_t redArg;
  uint64_t winBeg, winEnd;      // the bytes this launch covers, as FlatParams'
  const nexrFlatTreePart* ext;  // non-null: the parts are there, not in parts[]
  int nRanks, userFirst, preOp, postOp, nParts;
  int nOut;  // out[0 .. nOut) are stored
  FlatTreeProgram prog[2];
  nexrFlatTreePart parts[kFlatTreeInlineParts];
};
static_assert(sizeof(FlatTreeParams) <= 4000, "kernel argument block");
// nexrFlatTreeAllReducePreMul: FlatTreeParams' fields by the same names, PreMulSum implied, and the scalars as
// FlatPreMulParams carries them. FlatTreeParams is 3,904 bytes with 96 inline parts: 64 more 8-byte entries fit
// only with fewer of those, kFlatTreePreMulInlineParts; longer lists go to `ext` as they do already.
constexpr int kFlatTreePreMulInlineParts = NEXR_FLAT_TREE_PREMUL_INLINE_PARTS;
struct FlatTreePreMulParams {
  static constexpr bool kPerRank = true;
  const char* in[NEXR_SYM_MAX_RANKS];
  char* out[NEXR_SYM_MAX_RANKS];
  uint64_t scalars[NEXR_SYM_MAX_RANKS];
  uint64_t nBytes;
  uint64_t winBeg, winEnd;
  const nexrFlatTreePart* ext;
  int nRanks, userFirst, preOp, postOp, nParts;
  int nOut;
  int scalarsArePtrs, pad;
  FlatTreeProgram prog[2];
  nexrFlatTreePart parts[kFlatTreePreMulInlineParts];
};
static_assert(sizeof(FlatTreePreMulParams) <= 4000, "kernel argument block");
hipError_t launch_flat_tree_premul(int dt, const FlatTreePreMulParams& p, unsigned grid, hipStream_t s);
struct FlatTreePartsFill {
  nexrFlatTreePart* dst;
  int n, pad;
  nexrFlatTreePart parts[kFlatTreeInlineParts];
};
struct FlatBcastParams {
  const char* in;
  char* out[NEXR_SYM_MAX_RANKS];  // null: not written (its address is the input's)
  uint64_t nBytes;
  uint64_t winBeg, winEnd;  // the bytes this launch covers, as FlatParams'
  int nRanks, pad;
};
hipError_t launch_flat_tree(int dt, int op, const FlatTreeParams& p, unsigned grid, hipStream_t s);
hipError_t launch_flat_tree_parts(const FlatTreePartsFill& f, hipStream_t s);
hipError_t launch_flat_bcast(const FlatBcastParams& p, unsigned grid, hipStream_t s);

// Several flat collectives in one launch (nexrFlatGroup; nexr_flat_group.hip). A launch runs a table of works
// of one (datatype, device op, min-or-max): nWorks records of kFlatGroupRecBytes + 16 * nRanks bytes,
//   +0 itemEnd (the launch's items up to and including this work: its pieces, times nRanks for a reduce-scatter)
//   +8 regionBytes  +16 redArg  +24 coll  +28 root  +32 nParts  +36 partsAt (first part's index in the pool)
//   +40 in[nRanks]  then out[nRanks]
// then, at byte poolAt, the pool of the all-reduces' nexrFlatPart. The table rides in inl[] or, beyond it, in a
// stream-ordered workspace (`ext`) that flat_group_fill_kernel launches fill by value ahead of the launch. What
// the semantics make of the call (nFold, shift, preOp, postOp) holds for the whole launch.
constexpr int kFlatGroupInlineBytes = NEXR_FLAT_GROUP_INLINE_BYTES;
constexpr uint32_t kFlatGroupRecBytes = 40;
struct FlatGroupParams {
  const char* ext;  // non-null: the table is there, not in inl[]
  uint64_t nItems;
  int nWorks, nRanks;
  int nFold, shift, userFirst, preOp, postOp;  // as FlatParams'
  int isMin;                                   // nexrDevMinMax: the launch's direction
  uint32_t poolAt;
  int pad;
  char inl[kFlatGroupInlineBytes];
};
static_assert(sizeof(FlatGroupParams) <= 4000 && offsetof(FlatGroupParams, inl) % 8 == 0, "kernel argument block");
// Copies: records of kFlatGroupCopyRecBytes + 8 * maxOut bytes, {itemEnd, nBytes, src, dst[maxOut]}; a null
// destination is not written.
constexpr uint32_t kFlatGroupCopyRecBytes = 24;
struct FlatGroupCopyParams {
  const char* ext;
  uint64_t nItems;
  int nWorks, maxOut;
  char inl[kFlatGroupInlineBytes];
};
static_assert(sizeof(FlatGroupCopyParams) <= 4000 && offsetof(FlatGroupCopyParams, inl) % 8 == 0,
              "kernel argument block");
constexpr int kFlatGroupFillWords = NEXR_FLAT_GROUP_FILL_BYTES / 8;
struct FlatGroupFill {
  uint64_t* dst;
  int n, pad;
  uint64_t words[kFlatGroupFillWords];
};
static_assert(sizeof(FlatGroupFill) <= 4000, "kernel argument block");
hipError_t launch_flat_group(int dt, int op, const FlatGroupParams& p, unsigned grid, hipStream_t s);
hipError_t launch_flat_group_copy(const FlatGroupCopyParams& p, unsigned grid, hipStream_t s);
hipError_t launch_flat_group_fill(const FlatGroupFill& f, hipStream_t s);

// A batch of independent reduce-copies with the same (datatype, op, K) in one launch.
constexpr int kMaxBatch = 14;  // keeps the parameter block under the 4 KiB kernel-argument limit
struct BatchParams {
  int nWorks;
  uint32_t start[kMaxBatch + 1];  // work i owns workgroups [start[i], start[i+1])
  RCParams w[kMaxBatch];
};
static_assert(sizeof(BatchParams) <= 4000, "batch parameters must fit the kernel-argument segment");
static_assert(kMaxBatch == NEXR_MAX_BATCH_WORKS, "public batch limit must match the kernel's");

// Launch geometry chosen by the host.
struct Geometry {
  int grid;
  int pol;  // cache policy: 0 plain, 1 non-temporal loads, 3 non-temporal loads and stores
};

// One entry point per datatype, defined in the kernel object compiled with -DNEXR_DT=<dt>.
// Returns hipSuccess or the launch error.
#define NEXR_DECLARE_LAUNCH(dt) \
  hipError_t launch_dt##dt(const RCParams& p, int op, int nSrcs, const Geometry& g, hipStream_t s);
NEXR_DECLARE_LAUNCH(0) NEXR_DECLARE_LAUNCH(1) NEXR_DECLARE_LAUNCH(2) NEXR_DECLARE_LAUNCH(3)
NEXR_DECLARE_LAUNCH(4) NEXR_DECLARE_LAUNCH(5) NEXR_DECLARE_LAUNCH(6) NEXR_DECLARE_LAUNCH(7)
NEXR_DECLARE_LAUNCH(8) NEXR_DECLARE_LAUNCH(9)
#undef NEXR_DECLARE_LAUNCH
#define NEXR_DECLARE_BATCH(dt) \
  hipError_t launch_batch_dt##dt(const BatchParams& b, int op, int nSrcs, int pol, int grid, hipStream_t s);
NEXR_DECLARE_BATCH(0) NEXR_DECLARE_BATCH(1) NEXR_DECLARE_BATCH(2) NEXR_DECLARE_BATCH(3)
NEXR_DECLARE_BATCH(4) NEXR_DECLARE_BATCH(5) NEXR_DECLARE_BATCH(6) NEXR_DECLARE_BATCH(7)
NEXR_DECLARE_BATCH(8) NEXR_DECLARE_BATCH(9)
#undef NEXR_DECLARE_BATCH

// Workgroup geometry per (datatype, fan-in, cache policy): U packs per lane x B lanes per workgroup,
// and how many workgroups per CU the launch admits (lds_for; 0: as the registers allow). A workgroup owns one trip
// of U x B packs of every buffer, so the one-shot grid is nPacks / (U x B). U = 4, B = 256 is the default
// (round-1 steady-state sweeps over U in {1,2,4,8} x B in {256,512,1024} x occupancy caps for K = 2, 4, 8:
// profiles/r01_tune_*.log, r01_skew.log, r01s2_geom_*.log). The exceptions, each measured in one process
// against the alternatives on several boxes with byte-identical outputs:
//   - K = 4 with non-temporal loads and cached stores (64-512 MiB streamed, C4's regime), 1-, 2- and
//     8-byte types: U = 2, B = 512 — +0.9 % on average over 9 datatypes x {sum, min} on four boxes in
//     round 2 (profiles/r02_geom_sweep_*.log); with the round-5 body +0.9-3.6 % for int8, fp16 and bf16,
//     equal for uint64, and at one or two workgroups per CU 1-18 % slower; 4-byte types keep 4 x 256,
//     0.7-3.0 % faster with the round-5 body (int32 min at 16-100 MiB, int32 prod, fp32 sum;
//     profiles/r05s_occupancy_c4sizes.txt, r05t_occupancy_c4types.txt, r05l_occupancy_k8lanes.txt);
//   - the nt-store policy (>= 512 MiB streamed), where a CU's loads in flight are the lever (round 5,
//     tools/occupancy_ab.hip, profiles/r05b_occupancy_ab.txt, r05i_occupancy_wide.txt,
//     r05k_occupancy_k8shape.txt, r05l_occupancy_k8lanes.txt): the fastest point is about 64 KiB of
//     loads in flight per CU, i.e. 4096 / K lanes with one pack each, at ONE workgroup per CU
//       K = 4-5 (every type but fp16, mixed there at K = 4): U = 1, B = 1024 — at K = 4 4.2 % faster than
//         the two workgroups per CU its registers allow and +0.5-4 % over 4 x 256
//         (profiles/r02_geom_sweep_*); at K = 5 3.3-3.4 % over 4 x 256 (fp32, bf16, 1.5 GiB streamed;
//         profiles/r05zp_occupancy_k35.txt). bf16 alone takes two 512-lane workgroups per CU instead (round
//         6, with its hardware-RNE fold): 1.4-3.2 % faster at K = 4 and 2.8 % at K = 5 on two boxes, where
//         fp32, fp64, int32 and int8 lose 1.0-3.5 % that way (profiles/r06a_bf16cvt.txt, r06b_k45.txt).
//         K = 3 keeps 4 x 256: 1 x 1024 gained 2.9 % at 1 GiB with one
//         destination but lost 1.2-5.8 % at 96-300 MiB with 2-5 (profiles/r05zr_occupancy_k3m.txt), where
//         the nt-store table of pickPolicy (nexr_api.cpp) puts those calls under this policy;
//       K >= 6: U = 1, B = 512 — fp16 K = 8 2.5-2.7 % and fp32 K = 8 3.6 % faster than 1 x 1024, fp32
//         K = 6 1.3 %; 256 lanes are 10-20 % slower, 384 or 640 lanes 2 % slower. bf16 too since round 6:
//         with the hardware RNE (v_cvt_pk_bf16_f32, nexr_types.hpp) its fold no longer needs 1024 lanes
//         to hide it, and 1 x 512 is 1.6 % faster than the round-5 fold at 1 x 1024 and level with fp16
//         and a bare uint32 stream of the same bytes (profiles/r06a_bf16cvt.txt);
//   - 16-bit floats, K >= 8, below the nt-store policy: U = 1, B = 1024 as the registers admit (two per
//     CU): rounds 1 and 5 chose 1 x 1024 over 4 x 256 (profiles/r01s3_*_geometry_ab.txt); held to one
//     workgroup per CU it is 3.2-9.3 % slower under nt loads (64-512 MiB streamed) and equal under plain
//     (profiles/r05zm_occupancy_k8mid.txt) — the reservation pays only under nt stores (above).
// K = 2 keeps the default everywhere (U = 1 loses 10-13 %, U = 2 loses 1-5 %; 2 to 8 workgroups per CU
// are flat, profiles/r05b_occupancy_ab.txt).
constexpr int kTripPacks = 1024;  // the default trip (4 x 256)
struct Shape {
  int u, b;
  int wgsPerCu;  // 0: as the registers allow; 1 or 2: held there by an LDS reservation (lds_for)
};
__host__ __device__ constexpr Shape shape_for(int dt, int k, int pol) {
  const bool half = dt == nexrFloat16 || dt == nexrBfloat16;
  const bool four = dt == nexrInt32 || dt == nexrUint32 || dt == nexrFloat32;
  return (pol == 3 && k >= 6)                       ? Shape{1, 512, 1}
         : (half && k >= 8)                         ? Shape{1, 1024, 0}
         : (k == 4 && pol == 1 && !four)            ? Shape{2, 512, 0}
         : (k >= 4 && k <= 5 && pol == 3 && dt == nexrBfloat16) ? Shape{1, 512, 2}
         : (k >= 4 && k <= 5 && pol == 3 && dt != nexrFloat16) ? Shape{1, 1024, 1}
                                                    : Shape{4, 256, 0};
}
__host__ __device__ constexpr int unroll_for(int dt, int k, int pol) { return shape_for(dt, k, pol).u; }
__host__ __device__ constexpr int block_for(int dt, int k, int pol) { return shape_for(dt, k, pol).b; }
// n workgroups per CU: the launch reserves this many bytes of dynamic LDS (the kernel never touches
// it), so that only n fit in a CU's 160 KiB whatever the kernel's registers would admit.
constexpr int kLdsOneWorkgroupPerCu = 120 * 1024;  // one per CU (160 / 2 < 120 <= 160)
constexpr int kLdsTwoWorkgroupsPerCu = 66 * 1024;  // two per CU (160 / 3 < 66 <= 160 / 2)
__host__ __device__ constexpr int lds_for(int dt, int k, int pol) {
  return shape_for(dt, k, pol).wgsPerCu == 1   ? kLdsOneWorkgroupPerCu
         : shape_for(dt, k, pol).wgsPerCu == 2 ? kLdsTwoWorkgroupsPerCu
                                              : 0;
}

// The reduce-copy kernels that are compiled (round 6). Every other (datatype, op, K) is routed by the
// host onto one of them with the same bytes (routeKernel, nexr_api.cpp), so it is never launched:
//   - K = 1 without arithmetic (no pre-op scalar, no post-op divide) is a byte copy: uint8 Sum;
//   - signed integers' Sum, Prod, PreMulSum and SumPostDiv run the unsigned type's kernels (wrapping
//     two's-complement arithmetic, the reference's own equivalent_primary, generate.py:128-136; the
//     divide reads its signedness from redOpArg), so the signed objects hold Min / Max only;
//   - PreMulSum without pre-op sources and SumPostDiv without the divide are Sum.
// Batch launches are compiled for the plain and non-temporal-load policies only: a batch that would
// stream enough for non-temporal stores (>= 512 MiB) runs its works as single launches, where one launch
// per work costs nothing measurable against the work itself.
__host__ __device__ constexpr bool is_signed_int(int dt) { return dt == nexrInt8 || dt == nexrInt32 || dt == nexrInt64; }
__host__ __device__ constexpr bool kernel_compiled(int dt, int op, int k) {
  return k == 1 ? (op == nexrDevSum && dt == nexrUint8) ||
                      (!is_signed_int(dt) && (op == nexrDevPreMulSum || op == nexrDevSumPostDiv))
                : !is_signed_int(dt) || op == nexrDevMinMax;
}
constexpr int kBatchPolicies = 2;  // plain (0) and non-temporal loads (1)

}  // namespace nexr
